"""The switch of the read filter through the layers, without a GPU: ``ReadFilter``'s ranges and ``need_read_filter``;
with stubs, every route hands the keyword on only when it is set, and the streamed pair route asks for the full FASTQ
cut only then; the counters carry the filter's seven keys at the end of those in front of the filter counts, and are
exactly today's without a filter; the command line's options down to ``scan_report``."""
import dataclasses
import inspect
from contextlib import contextmanager

import pytest

from genefuserust_amd import multi_csv_scan, read_filter, scan, scan_stream
from genefuserust_amd.read_filter import COUNTER_KEYS, ReadFilter, need_read_filter
from tests.test_scan_pieces import FILTER_KEYS, ROUTES, TOT, _Mapper

TOTALS = [300, 250, 20, 333, 10, 20, 12, 8]
COUNTED = dict(zip(COUNTER_KEYS, TOTALS[1:]))


def test_the_settings_and_their_ranges():
    s = ReadFilter()
    assert dataclasses.astuple(s) == (10, 0, 20, 15, 5, 15, 40)
    assert [f.name for f in dataclasses.fields(s)] == ["poly_g_min", "cut_tail_window", "cut_tail_mean", "length_required",
                                                       "n_base_limit", "qualified_phred", "unqualified_percent"]
    with pytest.raises(dataclasses.FrozenInstanceError):
        s.poly_g_min = 3
    ReadFilter(0, 0, 0, 0, 0, 0, 0)
    ReadFilter(4096, 64, 93, 4096, 10 ** 9, 93, 100)
    for bad in (dict(poly_g_min=-1), dict(poly_g_min=4097), dict(cut_tail_window=65), dict(cut_tail_window=-1),
                dict(cut_tail_mean=94), dict(cut_tail_mean=-2), dict(length_required=4097), dict(length_required=-1),
                dict(n_base_limit=-1), dict(qualified_phred=94), dict(qualified_phred=-1), dict(unqualified_percent=101),
                dict(unqualified_percent=-1), dict(poly_g_min=2.5), dict(cut_tail_window="4"), dict(n_base_limit=True),
                dict(n_base_limit=None)):
        with pytest.raises(ValueError, match="ReadFilter.%s" % list(bad)[0]):
            ReadFilter(**bad)


def test_need_read_filter():
    s = ReadFilter(cut_tail_window=4)
    assert need_read_filter(None) is None and need_read_filter(s) is s
    for bad in (True, False, "defaults", 4, {}, (10, 0, 20, 15, 5, 15, 40), ReadFilter):
        with pytest.raises(ValueError, match="read_filter"):
            need_read_filter(bad)


def test_totals_as_counters():
    assert read_filter.totals_counters(TOTALS) == COUNTED and list(read_filter.totals_counters(TOTALS)) == list(COUNTER_KEYS)
    assert COUNTER_KEYS == ("reads_passed", "reads_trimmed", "bases_trimmed", "reads_too_short", "reads_too_many_n",
                            "reads_low_quality", "reads_mate_failed")


def test_the_keyword_is_keyword_only_on_every_route():
    for fn in (scan.scan_pair_end_files, scan.scan_pair_end_report, scan.scan_single_end_files,
               scan.scan_single_end_report, scan.streamed_found, multi_csv_scan.scan_multi_csv_report,
               multi_csv_scan.scan_report, multi_csv_scan._stream_multi_csv, scan_stream.scan_pair_source_stream,
               scan_stream.scan_single_text_stream, scan_stream._scan_source_stream, scan_stream._scan_chunk):
        p = inspect.signature(fn).parameters["read_filter"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn.__name__


def test_the_file_level_scans_check_the_keyword_before_any_file_is_opened():
    pair, single = ("no.fa", "no.csv", "r1.fq", "r2.fq"), ("no.fa", "no.csv", "r1.fq")
    for call, files in ((scan.scan_pair_end_files, pair), (scan.scan_pair_end_report, pair),
                        (scan.scan_single_end_files, single), (scan.scan_single_end_report, single),
                        (multi_csv_scan.scan_report, pair), (multi_csv_scan.scan_report, single),
                        (multi_csv_scan.scan_report, ("no.fa", "no.txt", "r1.fq", "r2.fq")),
                        (multi_csv_scan.scan_multi_csv_report, ("no.fa", "no.txt", "r1.fq", "r2.fq"))):
        with pytest.raises(ValueError, match="read_filter"):
            call(*files, read_filter="defaults")
        with pytest.raises(ValueError, match="read_filter"):
            call(*files, read_filter=True)


# ---- the counters -----------------------------------------------------------------------------------------------------

class _Totals:
    """The totals tensor as far as ``scan.filtered_reads`` looks."""

    def cpu(self):
        return self

    def tolist(self):
        return list(TOTALS)


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_counters_with_and_without_a_filter_keys_and_order(route, monkeypatch):
    _, (count_key, tot, chunks), front, back = route
    found = [b"a", b"drop", b"b"]
    calls = []

    def stub(ix, config, *batches):
        calls.append((ix, config, batches))
        return tuple("kept " + b for b in batches) + (_Totals(),)
    monkeypatch.setattr(read_filter, "filter_reads_device", stub)
    cfg = ReadFilter(cut_tail_window=4)
    kept, counted = scan.filtered_reads("ix", cfg, "l", "r")
    assert kept == ("kept l", "kept r") and calls == [("ix", cfg, ("l", "r"))]
    produced = counted((found, *scan.route_counters(count_key, 150, len(found), tot, chunks)))
    _, counters = scan.finish_matches(produced[0], _Mapper(), 50, False, *produced[1:])
    assert list(counters) == front + list(COUNTER_KEYS) + FILTER_KEYS + back
    assert {k: counters[k] for k in COUNTER_KEYS} == COUNTED and counters[count_key] == 150
    # without a filter: nothing is called, the batches are the same objects, the counters exactly today's
    del calls[:]
    kept, counted = scan.filtered_reads("ix", None, "l", "r")
    assert kept == ("l", "r") and calls == []
    produced = counted((found, *scan.route_counters(count_key, 150, len(found), tot, chunks)))
    _, counters = scan.finish_matches(produced[0], _Mapper(), 50, False, *produced[1:])
    assert list(counters) == front + FILTER_KEYS + back


# ---- the routes hand the keyword on only when it is set -----------------------------------------------------------------

class _Indexer:
    m_fusion_seq = ()

    def close(self):
        pass


@contextmanager
def _open_index(*a, **k):
    yield _Indexer(), []


def _streamed_routes(monkeypatch):
    """scan.py's streamed routes with the index, the sources and the two streams stubbed: what each stream was given."""
    seen = []

    def stream(kind):
        def run(ix, *args, **kw):   # today's signature: whatever is not handed on is not there
            seen.append((kind, kw))
            tot = dict(TOT, **{("pairs" if kind == "pair" else "reads"): 10}, **(COUNTED if "read_filter" in kw else {}))
            yield "rec", b"", b"", [], tot
            yield "rec", b"", b"", [], tot
        return run
    monkeypatch.setattr(scan, "open_index", _open_index)
    monkeypatch.setattr(scan, "FusionMapper", lambda ix: _Mapper())
    monkeypatch.setattr(scan, "finish_pair_hits", lambda *a: [])
    monkeypatch.setattr(scan, "named_from_device", lambda hits, rec, names, *orig: [])
    monkeypatch.setattr(scan_stream, "open_fastq_sources", lambda opened, files, inflate="host": list(files))
    monkeypatch.setattr(scan_stream, "scan_pair_source_stream", stream("pair"))
    monkeypatch.setattr(scan_stream, "scan_single_text_stream", stream("single"))
    return seen


def test_streamed_routes_hand_the_keyword_on_only_when_set(monkeypatch):
    seen = _streamed_routes(monkeypatch)
    cfg = ReadFilter()
    _, counters = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", chunk_bytes=4096, read_filter=cfg)
    assert seen[-1] == ("pair", {"max_read_len": None, "read_filter": cfg})
    assert list(counters) == ["pairs", "matches_before_filtering", "merged_pairs", "retried_reads"] + list(COUNTER_KEYS) + \
        FILTER_KEYS + ["chunks"]
    assert counters["pairs"] == 20 and counters["reads_passed"] == 2 * COUNTED["reads_passed"]   # summed over the chunks
    _, counters = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", chunk_bytes=4096)
    assert seen[-1] == ("pair", {"max_read_len": None})
    assert list(counters) == ["pairs", "matches_before_filtering", "merged_pairs", "retried_reads"] + FILTER_KEYS + ["chunks"]
    _, counters = scan.scan_single_end_files("ref.fa", "x.csv", "a.fq", chunk_bytes=4096, read_filter=cfg)
    assert seen[-1] == ("single", {"max_read_len": None, "read_filter": cfg})
    assert list(counters) == ["reads", "matches_before_filtering"] + list(COUNTER_KEYS) + FILTER_KEYS + \
        ["retried_reads", "chunks"]
    scan.scan_single_end_files("ref.fa", "x.csv", "a.fq", chunk_bytes=4096, originals=True)
    assert seen[-1] == ("single", {"max_read_len": None, "originals": True})


def test_whole_file_routes_filter_between_the_cut_and_the_scan(monkeypatch):
    calls = []
    monkeypatch.setattr(scan, "open_index", _open_index)
    monkeypatch.setattr(scan, "FusionMapper", lambda ix: _Mapper())

    class _Batch(str):
        def max_read_len(self):
            return 7

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
        calls.append(("filter", config, batches))
        return tuple(_Batch("kept " + b) for b in batches) + (_Totals(),)

    def pairs_found(mapper, reads, max_len, scan_fn, originals=False):
        calls.append(("pairs", [b for b, _ in reads]))
        return [], *scan.route_counters("pairs", 5, 0, TOT)

    def single(name):
        def found(*args):
            calls.append((name, [a for a in args if isinstance(a, _Batch)]))
            return [], *scan.route_counters("reads", 5, 0, TOT if name == "device" else None)
        return found
    monkeypatch.setattr(scan, "FastqReaderPair", _Reader)
    monkeypatch.setattr(scan, "FastqReader", _Reader)
    monkeypatch.setattr(read_filter, "filter_reads_device", filtered)
    monkeypatch.setattr(scan, "pairs_found", pairs_found)
    monkeypatch.setattr(scan, "single_end_found", single("device"))
    monkeypatch.setattr(scan, "_single_end_host_found", single("host"))
    cfg = ReadFilter(poly_g_min=0)
    _, counters = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", read_filter=cfg)
    assert calls == [("filter", cfg, ("cut a.fq", "cut b.fq")), ("pairs", ["kept cut a.fq", "kept cut b.fq"])]
    assert {k: counters[k] for k in COUNTER_KEYS} == COUNTED
    del calls[:]
    scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq")
    assert calls == [("pairs", ["cut a.fq", "cut b.fq"])]
    for route in ("device", "host"):
        del calls[:]
        _, counters = scan.scan_single_end_files("ref.fa", "x.csv", "a.fq", route=route, read_filter=cfg)
        assert calls == [("filter", cfg, ("cut a.fq",)), (route, ["kept cut a.fq"])]
        assert {k: counters[k] for k in COUNTER_KEYS} == COUNTED
        del calls[:]
        _, counters = scan.scan_single_end_files("ref.fa", "x.csv", "a.fq", route=route)
        assert calls == [(route, ["cut a.fq"])] and not set(COUNTER_KEYS) & set(counters)


def test_the_streamed_pair_route_asks_for_the_full_cut_only_with_a_filter(monkeypatch):
    seen = []

    def source_stream(indexer, sources, chunk_bytes, max_read_len, names, scan_records=None, lean=None, **kw):
        seen.append((lean, kw))
        return iter(())
    monkeypatch.setattr(scan_stream, "_scan_source_stream", source_stream)
    cfg = ReadFilter()
    scan_stream.scan_pair_source_stream("ix", "r1", "r2", 4096)
    scan_stream.scan_pair_source_stream("ix", "r1", "r2", 4096, read_filter=cfg)
    scan_stream.scan_single_text_stream("ix", "r1", 4096)
    scan_stream.scan_single_text_stream("ix", "r1", 4096, read_filter=cfg)
    assert seen == [(None, {}), (False, {"read_filter": cfg}), (None, {}), (None, {"read_filter": cfg})]


def test_a_chunk_is_cut_the_full_way_filtered_then_scanned(monkeypatch):
    """``_scan_chunk``: with a filter the cut is the full one whatever ``lean`` says, the records the sides share go
    through the filter, the scan gets what it leaves, and the chunk's totals gain the seven counts."""
    from genefuserust_amd import fastq
    calls = []

    class _B:
        n_records, n_newlines = 3, 12

        def __init__(self, name):
            self.name = name

    monkeypatch.setattr(fastq, "fastq_cut_device", lambda ix, t, lean=False: (calls.append(("cut", t, lean)), _B(t))[1])
    monkeypatch.setattr(scan_stream, "_record_cuts", lambda batches, texts, final, names: (3, [3] * len(texts), [0] * len(texts)))

    def filter_chunk(ix, config, batches, m):
        calls.append(("filter", config, [b.name for b in batches], m))
        return ["kept " + b.name for b in batches], _Totals()
    monkeypatch.setattr(scan_stream, "_filter_chunk", filter_chunk)

    def scan_records(ix, texts, batches, m, done, max_read_len, names):
        calls.append(("scan", [b if isinstance(b, str) else b.name for b in batches]))
        return ("rec", b"", b"", [], {"pairs": m})
    cfg = ReadFilter()
    _, _, (out, m, last) = scan_stream._scan_chunk("ix", ["a", "b"], ["t1", "t2"], [False, False], 0, None, True,
                                                   scan_records, read_filter=cfg)
    assert calls == [("cut", "t1", False), ("cut", "t2", False), ("filter", cfg, ["t1", "t2"], 3),
                     ("scan", ["kept t1", "kept t2"])]
    assert out[4] == dict({"pairs": 3}, **COUNTED)
    # K indexes: every one's totals gain the same counts
    many = lambda *a: [("rec", b"", b"", [], {"pairs": 3}), ("rec", b"", b"", [], {"pairs": 3})]   # noqa: E731
    _, _, (out, _, _) = scan_stream._scan_chunk("ix", ["a", "b"], ["t1", "t2"], [False, False], 0, None, True, many,
                                                read_filter=cfg)
    assert [o[4] for o in out] == [dict({"pairs": 3}, **COUNTED)] * 2
    # without: today's call, the lean cut for pairs, no filter
    del calls[:]
    _, _, (out, _, _) = scan_stream._scan_chunk("ix", ["a", "b"], ["t1", "t2"], [False, False], 0, None, True, scan_records)
    assert calls == [("cut", "t1", True), ("cut", "t2", True), ("scan", ["t1", "t2"])] and out[4] == {"pairs": 3}


def test_scan_report_hands_the_keyword_on_only_when_set(monkeypatch):
    seen = []
    monkeypatch.setattr(scan, "scan_pair_end_report", lambda *a, **k: (seen.append(("pair", k)), ([], {}))[1])
    monkeypatch.setattr(scan, "scan_single_end_report", lambda *a, **k: (seen.append(("single", k)), ([], {}))[1])
    monkeypatch.setattr(multi_csv_scan, "scan_multi_csv_report", lambda *a, **k: (seen.append(("multi", k)), [])[1])
    cfg = ReadFilter(n_base_limit=0)
    for files in (("ref.fa", "x.csv", "r1.fq", "r2.fq"), ("ref.fa", "x.csv", "r1.fq"), ("ref.fa", "list.txt", "r1.fq", "r2.fq")):
        multi_csv_scan.scan_report(*files, read_filter=cfg)
        multi_csv_scan.scan_report(*files)
    assert [w for w, _ in seen] == ["pair", "pair", "single", "single", "multi", "multi"]
    assert [k.get("read_filter", "absent") for _, k in seen] == [cfg, "absent"] * 3


def test_multi_csv_streamed_hands_the_keyword_on_only_when_set(monkeypatch):
    seen = []

    def source_stream(ix, sources, chunk_bytes, max_read_len, names, scan_records=None, lean=None, **kw):
        seen.append((lean, kw))
        tot = dict(TOT, pairs=4, **(COUNTED if kw else {}))
        yield [("rec", b"", b"", [], dict(tot)), ("rec", b"", b"", [], dict(tot))]
        yield [("rec", b"", b"", [], dict(tot)), ("rec", b"", b"", [], dict(tot))]
    monkeypatch.setattr(scan_stream, "_scan_source_stream", source_stream)
    monkeypatch.setattr(scan_stream, "open_fastq_sources", lambda opened, files, inflate="host": list(files))
    import genefuserust_amd.fusion_mapper as fusion_mapper
    import genefuserust_amd.read_pair as read_pair
    monkeypatch.setattr(fusion_mapper, "FusionMapper", lambda ix: _Mapper())
    monkeypatch.setattr(read_pair, "finish_pair_hits", lambda *a: [])
    monkeypatch.setattr(scan, "named_from_device", lambda hits, rec, names, *orig: [])
    cfg = ReadFilter()
    out = multi_csv_scan._stream_multi_csv(["ix0", "ix1"], ("a.fq", "b.fq"), 4096, read_filter=cfg)
    assert seen[-1] == (False, {"read_filter": cfg})
    for _, before, after in out:   # every CSV reports the same totals, summed over the chunks
        assert list(before) == ["pairs", "matches_before_filtering", "merged_pairs", "retried_reads"] + list(COUNTER_KEYS)
        assert {k: before[k] for k in COUNTER_KEYS} == {k: 2 * v for k, v in COUNTED.items()} and after == {"chunks": 2}
    out = multi_csv_scan._stream_multi_csv(["ix0", "ix1"], ("a.fq", "b.fq"), 4096)
    assert seen[-1] == (False, {})
    assert [list(before) for _, before, _ in out] == [["pairs", "matches_before_filtering", "merged_pairs", "retried_reads"]] * 2


# ---- the command line -------------------------------------------------------------------------------------------------

def test_the_command_line_options_reach_scan_report(monkeypatch, tmp_path, capsys):
    from genefuserust_amd import cli
    base = ["-1", "a.fq", "-f", "x.csv", "-r", "ref.fa"]
    a = cli.parser().parse_args(base)
    assert a.read_filter is False and all(getattr(a, k) is None for k in cli.READ_FILTER_OPTIONS)
    assert cli._read_filter(a) is None
    assert cli._read_filter(cli.parser().parse_args(base + ["--read-filter"])) == ReadFilter()
    options = {"--qualified-phred": ("qualified_phred", 20), "--unqualified-percent": ("unqualified_percent", 30),
               "--n-base-limit": ("n_base_limit", 2), "--length-required": ("length_required", 36),
               "--cut-tail-window": ("cut_tail_window", 4), "--cut-tail-mean": ("cut_tail_mean", 25),
               "--poly-g-min": ("poly_g_min", 0)}
    assert sorted(f for f, _ in options.values()) == sorted(f.name for f in dataclasses.fields(ReadFilter))
    for option, (field, value) in options.items():   # each sets its field, and implies the switch
        assert cli._read_filter(cli.parser().parse_args(base + [option, str(value)])) == ReadFilter(**{field: value})
    every = [x for option, (_, value) in options.items() for x in (option, str(value))]
    assert cli._read_filter(cli.parser().parse_args(base + every + ["--read-filter"])) == \
        ReadFilter(**{f: v for f, v in options.values()})
    seen = []

    def scan_report(ref, fusion, r1, r2, **kw):
        seen.append(("one", kw))
        return [], {}

    def scan_multi_csv_report(ref, fusion, r1, r2, **kw):
        seen.append(("streamed list", kw))
        return []
    monkeypatch.setattr(multi_csv_scan, "scan_report", scan_report)
    monkeypatch.setattr(multi_csv_scan, "scan_multi_csv_report", scan_multi_csv_report)
    for name in ("ref.fa", "x.csv", "panels.txt", "a.fq", "b.fq"):
        (tmp_path / name).write_text("")
    files = ["-1", str(tmp_path / "a.fq"), "-2", str(tmp_path / "b.fq"), "-r", str(tmp_path / "ref.fa"), "-h", "", "-j", ""]
    csv, lst = ["-f", str(tmp_path / "x.csv")], ["-f", str(tmp_path / "panels.txt")]
    assert cli.main(files + csv) == 0 and "read_filter" not in seen[-1][1]                # off: the call of today
    assert cli.main(files + csv + ["--read-filter"]) == 0 and seen[-1][1]["read_filter"] == ReadFilter()
    assert cli.main(files + csv + ["--cut-tail-window", "4"]) == 0
    assert seen[-1][1]["read_filter"] == ReadFilter(cut_tail_window=4)
    assert cli.main(files + lst + ["--read-filter", "--poly-g-min", "12"]) == 0
    assert seen[-1] == ("one", dict(seen[-1][1], read_filter=ReadFilter(poly_g_min=12)))
    assert cli.main(files + lst + ["--chunk-bytes", "4096", "--n-base-limit", "1"]) == 0
    assert seen[-1][0] == "streamed list" and seen[-1][1]["read_filter"] == ReadFilter(n_base_limit=1)
    assert cli.main(files + lst + ["--chunk-bytes", "4096"]) == 0 and "read_filter" not in seen[-1][1]
    capsys.readouterr()
    # a value out of range ends the run with a message, before the scan
    count = len(seen)
    assert cli.main(files + csv + ["--cut-tail-window", "65"]) == 1 and len(seen) == count
    assert "ReadFilter.cut_tail_window" in capsys.readouterr().err
