"""The switch of the duplicate removal through the layers, without a GPU: ``need_dedup`` and the values ``Dedup``
refuses; the keyword on every route that has ``read_filter``, checked before a file is opened; with stubs, every route
hands it on only when it is set, the counters' order with and without trimming and filter, a streamed chunk offers the
records the sides share and not the batch; when the table grows, at exactly half full and one past, and ``max_slots``;
the command line's options down to ``scan_report``; and the QC document with and without ``duplication``."""
import inspect
import json
from contextlib import contextmanager

import numpy as np
import pytest

from genefuserust_amd import cli, multi_csv_scan, read_qc, scan, scan_stream
from genefuserust_amd.adapter_trim import ADAPTER_COUNTER_KEYS, AdapterTrim
from genefuserust_amd.dedup import DEDUP_COUNTER_KEYS, Dedup, DedupResult, dedup_totals_counters, need_dedup
from genefuserust_amd.read_filter import COUNTER_KEYS, ReadFilter
from tests.test_scan_pieces import TOT, _Mapper


def test_need_dedup_and_bad_values():
    d = Dedup()
    assert need_dedup(None) is None and need_dedup(d) is d
    assert (d.remove, d.slots, d.max_slots, d.offered) == (True, 1 << 22, 1 << 31, 0)
    for bad in (True, False, "on", 1, {}, Dedup):
        with pytest.raises(ValueError, match="dedup must be None or a Dedup"):
            need_dedup(bad)
    for bad in (None, 1, "no"):
        with pytest.raises(ValueError, match="remove"):
            Dedup(remove=bad)
    for bad in (0, -1024, 512, 1000, 1025, 3 << 20, 2.0 ** 20, "1024", True, None):
        with pytest.raises(ValueError, match="slots must be a power of two"):
            Dedup(slots=bad)
        with pytest.raises(ValueError, match="max_slots must be a power of two"):
            Dedup(max_slots=bad)
    with pytest.raises(ValueError, match="below slots"):
        Dedup(slots=4096, max_slots=2048)
    assert Dedup(slots=1024, max_slots=1024).slots == 1024
    assert d.result() == DedupResult(0, 0, 0, 0, (0,) * 32) and d.result().rate() == 0.0   # nothing offered, no device
    doc = Dedup.__doc__
    assert "two lanes" in doc and "same file twice" in doc


def test_totals_counters():
    assert dedup_totals_counters([10, 9, 4, 5, 700, 0]) == dict(zip(DEDUP_COUNTER_KEYS, (9, 4, 5, 700)))
    # nothing removed: the duplicates are the hashed records less the new keys, and no base is counted
    assert dedup_totals_counters([10, 9, 4, 0, 0, 0], remove=False) == dict(zip(DEDUP_COUNTER_KEYS, (9, 4, 5, 0)))


def test_growth_decisions():
    """The table grows before an insert that could take it past half full: offered + n > slots / 2."""
    d = Dedup(slots=1024, max_slots=1 << 14)
    assert d.slots_for(0) == d.slots_for(512) == 1024          # exactly half full: it stays
    assert d.slots_for(513) == 2048                            # one past: the next power of two
    assert d.slots_for(1024) == 2048 and d.slots_for(1025) == 4096 and d.slots_for(8192) == 1 << 14
    d.offered = 500
    assert d.slots_for(12) == 1024 and d.slots_for(13) == 2048 and d.slots_for(1549) == 8192
    with pytest.raises(RuntimeError, match=r"500 records offered and 7693 more need a table of 32768 slots; max_slots "
                                           r"is 16384"):
        d.slots_for(7693)
    assert d.slots_for(7692) == 1 << 14 and d.slots == 1024   # asking changes nothing


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
    assert len(routes) == 14
    for fn in routes:
        p = inspect.signature(fn).parameters["dedup"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn.__name__


def test_the_file_level_scans_check_the_keyword_before_any_file_is_opened():
    pair, single = ("no.fa", "no.csv", "r1.fq", "r2.fq"), ("no.fa", "no.csv", "r1.fq")
    for call, files in ((scan.scan_pair_end_files, pair), (scan.scan_pair_end_report, pair),
                        (scan.scan_single_end_files, single), (scan.scan_single_end_report, single),
                        (multi_csv_scan.scan_report, pair), (multi_csv_scan.scan_report, single),
                        (multi_csv_scan.scan_report, ("no.fa", "no.txt", "r1.fq", "r2.fq")),
                        (multi_csv_scan.scan_multi_csv_report, ("no.fa", "no.txt", "r1.fq", "r2.fq"))):
        for bad in ("yes", True):
            with pytest.raises(ValueError, match="dedup must be None or a Dedup"):
                call(*files, dedup=bad)
    for call in (scan_stream.scan_pair_source_stream, scan_stream.scan_single_text_stream):
        with pytest.raises(ValueError, match="dedup must be None or a Dedup"):
            call("ix", *(("r1", "r2") if call is scan_stream.scan_pair_source_stream else ("r1",)), dedup=True)


# ---- the routes hand the keyword on only when it is set -----------------------------------------------------------------

class _Totals:
    def __init__(self, values):
        self.values = list(values)

    def cpu(self):
        return self

    def tolist(self):
        return self.values


class _Dedup(Dedup):
    """A collector that only writes down what it is offered."""

    def __init__(self, remove=True):
        super().__init__(remove=remove)
        self.calls = []

    def apply(self, indexer, *batches, stream=None):
        self.calls.append(batches)
        return tuple(_Batch("unique " + b) if isinstance(b, str) else b for b in batches), _Totals([5, 5, 3, 2, 300, 0])


class _Batch(str):
    def max_read_len(self):
        return 7


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
            tot = dict(TOT, **{("pairs" if kind == "pair" else "reads"): 10})
            if "dedup" in kw:
                tot.update(dict(zip(DEDUP_COUNTER_KEYS, (9, 4, 5, 700))))
            yield "rec", b"", b"", [], tot
        return run
    monkeypatch.setattr(scan, "open_index", _open_index)
    monkeypatch.setattr(scan, "FusionMapper", lambda ix: _Mapper())
    monkeypatch.setattr(scan, "finish_pair_hits", lambda *a: [])
    monkeypatch.setattr(scan, "named_from_device", lambda hits, rec, names, *orig: [])
    monkeypatch.setattr(scan_stream, "open_fastq_sources", lambda opened, files, inflate="host": list(files))
    monkeypatch.setattr(scan_stream, "scan_pair_source_stream", stream("pair"))
    monkeypatch.setattr(scan_stream, "scan_single_text_stream", stream("single"))
    d = _Dedup()
    _, with_dedup = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", chunk_bytes=4096, dedup=d)
    assert seen[-1] == ("pair", {"max_read_len": None, "dedup": d})
    _, without = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", chunk_bytes=4096)
    assert seen[-1] == ("pair", {"max_read_len": None})
    # the four counters, in front of the filter counts; everything else stays
    keys = list(with_dedup)
    at = keys.index("dedup_checked")
    assert tuple(keys[at:at + 4]) == DEDUP_COUNTER_KEYS and keys[:at] + keys[at + 4:] == list(without)
    assert keys[at - 1] == "retried_reads" and keys[at + 4] == list(without)[at]
    assert {k: with_dedup[k] for k in DEDUP_COUNTER_KEYS} == dict(zip(DEDUP_COUNTER_KEYS, (9, 4, 5, 700)))
    scan.scan_single_end_report("ref.fa", "x.csv", "a.fq", chunk_bytes=4096, dedup=d)
    assert seen[-1] == ("single", {"max_read_len": None, "dedup": d})
    scan.scan_single_end_report("ref.fa", "x.csv", "a.fq", chunk_bytes=4096)
    assert seen[-1] == ("single", {"max_read_len": None})


def _whole_file_stubs(monkeypatch, calls):
    monkeypatch.setattr(scan, "open_index", _open_index)
    monkeypatch.setattr(scan, "FusionMapper", lambda ix: _Mapper())

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
        return tuple(_Batch("kept " + b) for b in batches) + (_Totals([0] * 8),)

    def trimmed(ix, config, *batches):
        calls.append(("trim", batches))
        return tuple(_Batch("cut-to-insert " + b) for b in batches) + (_Totals([0] * 6),)

    def found(kind, key):
        def run(*args, **kw):
            calls.append((kind,))
            return [], *scan.route_counters(key, 5, 0, TOT)
        return run
    from genefuserust_amd import adapter_trim, read_filter
    monkeypatch.setattr(scan, "FastqReaderPair", _Reader)
    monkeypatch.setattr(scan, "FastqReader", _Reader)
    monkeypatch.setattr(read_filter, "filter_reads_device", filtered)
    monkeypatch.setattr(adapter_trim, "trim_adapters_device", trimmed)
    monkeypatch.setattr(scan, "pairs_found", found("pairs", "pairs"))
    monkeypatch.setattr(scan, "single_end_found", found("device", "reads"))
    monkeypatch.setattr(scan, "_single_end_host_found", found("host", "reads"))


def test_whole_file_routes_deduplicate_last_and_count_behind_the_filter(monkeypatch):
    calls = []
    _whole_file_stubs(monkeypatch, calls)
    d, cfg, trim = _Dedup(), ReadFilter(), AdapterTrim()
    qc = read_qc.ReadQc()
    qc.measure = lambda ix, stage, *b, stream=None: calls.append((stage, b))
    _, counters = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", read_filter=cfg, adapter_trim=trim,
                                           dedup=d, qc=qc)
    kept = ("kept cut-to-insert cut a.fq", "kept cut-to-insert cut b.fq")
    assert d.calls == [kept]
    # "after" is measured behind the duplicate removal
    assert calls == [("before", ("cut a.fq", "cut b.fq")), ("trim", ("cut a.fq", "cut b.fq")),
                     ("filter", ("cut-to-insert cut a.fq", "cut-to-insert cut b.fq")),
                     ("after", tuple("unique " + k for k in kept)), ("pairs",)]
    keys = list(counters)
    at = keys.index(ADAPTER_COUNTER_KEYS[0])
    assert tuple(keys[at:at + 16]) == ADAPTER_COUNTER_KEYS + COUNTER_KEYS + DEDUP_COUNTER_KEYS
    assert keys[at + 16] == "complexity" and counters["dedup_duplicates"] == 2 and counters["dedup_bases_removed"] == 300
    # without trimming and filter: the four keys alone, in the same place, and "after" is still measured
    del calls[:]
    _, alone = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", dedup=d, qc=qc)
    assert calls == [("before", ("cut a.fq", "cut b.fq")), ("after", ("unique cut a.fq", "unique cut b.fq")), ("pairs",)]
    _, plain = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq")
    keys = list(alone)
    at = keys.index("dedup_checked")
    assert tuple(keys[at:at + 4]) == DEDUP_COUNTER_KEYS and keys[:at] + keys[at + 4:] == list(plain)
    assert keys[at + 4] == "complexity"
    # counting only: the duplicates are the hashed records less the new keys
    _, counted = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", dedup=_Dedup(remove=False))
    assert [counted[k] for k in DEDUP_COUNTER_KEYS] == [5, 3, 2, 0]
    for route in ("device", "host"):
        del calls[:], d.calls[:]
        _, single = scan.scan_single_end_files("ref.fa", "x.csv", "a.fq", route=route, read_filter=cfg, dedup=d)
        assert calls == [("filter", ("cut a.fq",)), (route,)] and d.calls == [("kept cut a.fq",)]
        keys = list(single)
        at = keys.index(COUNTER_KEYS[0])
        assert tuple(keys[at:at + 11]) == COUNTER_KEYS + DEDUP_COUNTER_KEYS
        del calls[:], d.calls[:]
        scan.scan_single_end_files("ref.fa", "x.csv", "a.fq", route=route)
        assert calls == [(route,)] and d.calls == []


def test_the_streamed_routes_ask_for_the_full_cut_only_with_dedup(monkeypatch):
    seen = []

    def source_stream(indexer, sources, chunk_bytes, max_read_len, names, scan_records=None, lean=None, **kw):
        seen.append((lean, kw))
        return iter(())
    monkeypatch.setattr(scan_stream, "_scan_source_stream", source_stream)
    d = _Dedup()
    scan_stream.scan_pair_source_stream("ix", "r1", "r2", 4096)
    scan_stream.scan_pair_source_stream("ix", "r1", "r2", 4096, dedup=d)
    scan_stream.scan_single_text_stream("ix", "r1", 4096)
    scan_stream.scan_single_text_stream("ix", "r1", 4096, dedup=d)
    assert seen == [(None, {}), (False, {"dedup": d}), (None, {}), (None, {"dedup": d})]


class _B:
    """A batch of 5 records as far as ``_scan_chunk`` looks."""
    n_records, n_newlines = 5, 20

    def __init__(self, name, offsets=(0, 1, 2, 3, 4, 5)):
        self.name, self.offsets = name, list(offsets)

    def _replace(self, **kw):
        out = _B(self.name, kw["offsets"])
        out.n_records = kw["n_records"]
        return out


def test_a_chunk_offers_the_records_it_scans_never_the_ones_it_carries_over(monkeypatch):
    """``_scan_chunk``: with ``dedup`` the cut is the full one whatever ``lean`` says; the first m = 3 of a batch's 5
    records go through the filter and are then offered to the table; the scan gets what the removal leaves; the totals
    go behind the filter's, for one index and for a list of them."""
    from genefuserust_amd import fastq
    calls = []
    monkeypatch.setattr(fastq, "fastq_cut_device", lambda ix, t, lean=False: (calls.append(("cut", t, lean)), _B(t))[1])
    monkeypatch.setattr(scan_stream, "_record_cuts",
                        lambda batches, texts, final, names: (3, [5] * len(texts), [0] * len(texts)))

    def filter_chunk(ix, config, batches, m):
        calls.append(("filter", [b.name for b in batches], m))
        return [_B("kept " + b.name, b.offsets[:m + 1]) for b in batches], _Totals([0] * 8)
    monkeypatch.setattr(scan_stream, "_filter_chunk", filter_chunk)

    class _Chunks(_Dedup):
        def apply(self, indexer, *batches, stream=None):
            calls.append(("dedup", [(b.name, b.n_records, len(b.offsets)) for b in batches]))
            return tuple(_B("unique " + b.name, b.offsets) for b in batches), _Totals([3, 3, 2, 1, 150, 0])

    def scan_records(ix, texts, batches, m, done, max_read_len, names):
        calls.append(("scan", [b.name for b in batches], m))
        return ("rec", b"", b"", [], {"pairs": m})
    d = _Chunks()
    out = scan_stream._scan_chunk("ix", ["r1", "r2"], ["t1", "t2"], [False, False], 0, None, True, scan_records, True,
                                  read_filter=ReadFilter(), dedup=d)
    assert calls == [("cut", "t1", False), ("cut", "t2", False), ("filter", ["t1", "t2"], 3),
                     ("dedup", [("kept t1", 3, 4), ("kept t2", 3, 4)]), ("scan", ["unique kept t1", "unique kept t2"], 3)]
    tot = out[2][0][4]
    assert list(tot) == ["pairs"] + list(COUNTER_KEYS) + list(DEDUP_COUNTER_KEYS)
    assert [tot[k] for k in DEDUP_COUNTER_KEYS] == [3, 2, 1, 150]
    # alone, and a list of indexes: offered once, every index reports the same totals
    del calls[:]
    out = scan_stream._scan_chunk("ix", ["r1"], ["t1"], [False], 0, None, True,
                                  lambda *a: [scan_records(*a), scan_records(*a)], None, dedup=d)
    assert [c[0] for c in calls] == ["cut", "dedup", "scan", "scan"] and calls[0] == ("cut", "t1", False)
    assert calls[1] == ("dedup", [("t1", 3, 4)])
    assert [list(per_index[4]) for per_index in out[2][0]] == [["pairs"] + list(DEDUP_COUNTER_KEYS)] * 2
    # without it: the cut and the scan of today
    del calls[:]
    scan_stream._scan_chunk("ix", ["r1", "r2"], ["t1", "t2"], [False, False], 0, None, True, scan_records, True)
    assert calls == [("cut", "t1", True), ("cut", "t2", True), ("scan", ["t1", "t2"], 3)]


def test_multi_csv_hands_the_keyword_on_only_when_set(monkeypatch):
    seen = []

    def stream(indexers, files, chunk_bytes, hits_cap=None, inflate="host", originals=False, **kw):
        seen.append(kw)
        return []
    monkeypatch.setattr(multi_csv_scan, "_stream_multi_csv", stream)
    monkeypatch.setattr(multi_csv_scan, "read_csv_list", lambda path: [])
    from genefuserust_amd import scan as scan_module
    monkeypatch.setattr(scan_module, "read_contigs", lambda path: {})
    d = _Dedup()
    multi_csv_scan.scan_multi_csv_report("ref.fa", "list.txt", "a.fq", "b.fq", chunk_bytes=4096, dedup=d)
    multi_csv_scan.scan_multi_csv_report("ref.fa", "list.txt", "a.fq", "b.fq", chunk_bytes=4096)
    assert seen == []   # (no CSV, no index: nothing is streamed)
    calls = []
    monkeypatch.setattr(multi_csv_scan, "scan_multi_csv_report", lambda *a, **kw: calls.append(kw) or [])
    multi_csv_scan.scan_report("ref.fa", "list.txt", "a.fq", "b.fq", dedup=d)
    multi_csv_scan.scan_report("ref.fa", "list.txt", "a.fq", "b.fq")
    assert calls[0]["dedup"] is d and "dedup" not in calls[1]


# ---- the command line ---------------------------------------------------------------------------------------------------

def _args(*extra):
    return cli.parser().parse_args(["-1", "a.fq", "-f", "x.csv", "-r", "ref.fa", *extra])


def test_cli_options():
    assert cli._dedup(_args()) is None
    d = cli._dedup(_args("--dedup"))
    assert isinstance(d, Dedup) and d.remove and (d.slots, d.max_slots) == (1 << 22, 1 << 31)
    d = cli._dedup(_args("--dedup-count-only"))
    assert isinstance(d, Dedup) and not d.remove
    d = cli._dedup(_args("--dedup-max-slots", str(1 << 24)))
    assert d.remove and (d.slots, d.max_slots) == (1 << 22, 1 << 24)
    d = cli._dedup(_args("--dedup-max-slots", "4096", "--dedup-count-only"))
    assert not d.remove and (d.slots, d.max_slots) == (4096, 4096)
    for bad in ("1000", "512", "0", "3072"):
        with pytest.raises(ValueError, match="power of two"):
            cli._dedup(_args("--dedup-max-slots", bad))


def test_cli_hands_the_collector_to_the_scan_and_its_result_to_the_qc_report(monkeypatch, tmp_path):
    seen = []

    def scan_report(ref, fusion, r1, r2, **kw):
        seen.append(kw)
        return [], {"pairs": 0}
    monkeypatch.setattr(multi_csv_scan, "scan_report", scan_report)
    files = []
    for name in ("a.fq", "x.csv", "ref.fa"):
        (tmp_path / name).write_text("")
        files.append(str(tmp_path / name))
    base = ["-1", files[0], "-f", files[1], "-r", files[2], "-h", "", "-j", ""]
    assert cli.main(base) == 0 and "dedup" not in seen[-1]
    assert cli.main(base + ["--dedup"]) == 0 and isinstance(seen[-1]["dedup"], Dedup)
    assert cli.main(base + ["--dedup-max-slots", "1000"]) == 1
    qc_file = tmp_path / "qc.json"
    monkeypatch.setattr(Dedup, "result", lambda self: DedupResult(10, 6, 4, 0, (0, 4, 1, 1) + (0,) * 28))
    assert cli.main(base + ["--dedup-count-only", "--qc-json", str(qc_file)]) == 0
    doc = json.loads(qc_file.read_text())
    assert doc["duplication"] == {"rate": 0.4, "histogram": [4, 1, 1] + [0] * 28}
    assert cli.main(base + ["--qc-json", str(qc_file)]) == 0 and "duplication" not in json.loads(qc_file.read_text())


# ---- the QC document ----------------------------------------------------------------------------------------------------

def test_qc_document_with_and_without_duplication():
    tables = (np.zeros(read_qc.SIDE_WORDS, dtype=np.int64),)
    result = read_qc.QcResult(tables, tables, None)
    plain = read_qc.report_document(result)
    assert "duplication" not in plain and read_qc.report_json(result) == json.dumps(plain, indent=1) + "\n"
    hist = (0, 7, 2) + (0,) * 28 + (1,)
    doc = read_qc.report_document(result, None, DedupResult(50, 10, 40, 6000, hist))
    assert doc["duplication"] == {"rate": 0.8, "histogram": list(hist[1:])} and len(doc["duplication"]["histogram"]) == 31
    keys = list(doc)
    assert keys.index("summary") < keys.index("duplication") < keys.index("read1_before_filtering")
    assert {k: v for k, v in doc.items() if k != "duplication"} == plain
    assert read_qc.report_document(result, duplication=DedupResult(0, 0, 0, 0, (0,) * 32))["duplication"]["rate"] == 0.0
    assert json.loads(read_qc.report_json(result, None, DedupResult(50, 10, 40, 6000, hist))) == doc
