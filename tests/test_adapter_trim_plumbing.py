"""The switch of the adapter trimming through the layers, without a GPU: ``AdapterTrim`` and ``need_adapter_trim``;
with stubs, every route hands the keyword on only when it is set, and the streamed pair route asks for the full FASTQ
cut only then; the order is cut, trim, filter, scan; the counters carry the trimming's five keys in front of the read
filter's seven, in front of the filter counts, and are exactly today's with neither; the command line's options down to
``scan_report``."""
import dataclasses
import inspect
from contextlib import contextmanager

import pytest

from genefuserust_amd import adapter_trim, multi_csv_scan, read_filter, scan, scan_stream
from genefuserust_amd.adapter_trim import ADAPTER_COUNTER_KEYS, AdapterTrim, need_adapter_trim
from genefuserust_amd.read_filter import COUNTER_KEYS, ReadFilter
from tests.test_scan_pieces import FILTER_KEYS, ROUTES, TOT, _Mapper

TOTALS = [300, 120, 4000, 100, 20, 70]
COUNTED = dict(zip(ADAPTER_COUNTER_KEYS, TOTALS[1:]))
RF_TOTALS = [300, 250, 20, 333, 10, 20, 12, 8]
RF_COUNTED = dict(zip(COUNTER_KEYS, RF_TOTALS[1:]))
ALL_ROUTES = (scan.scan_pair_end_files, scan.scan_pair_end_report, scan.scan_single_end_files,
              scan.scan_single_end_report, scan.streamed_found, multi_csv_scan.scan_multi_csv_report,
              multi_csv_scan.scan_report, multi_csv_scan._stream_multi_csv, scan_stream.scan_pair_source_stream,
              scan_stream.scan_single_text_stream, scan_stream._scan_source_stream, scan_stream._scan_chunk)
PAIR_FRONT = ["pairs", "matches_before_filtering", "merged_pairs", "retried_reads"]


def test_the_settings():
    s = AdapterTrim()
    assert dataclasses.astuple(s) == (True, "", "", 30, 5, 20, 10)
    assert [f.name for f in dataclasses.fields(s)] == ["overlap", "adapter_r1", "adapter_r2", "min_overlap", "max_diff",
                                                       "diff_percent", "min_adapter"]
    with pytest.raises(dataclasses.FrozenInstanceError):
        s.min_overlap = 3
    both = AdapterTrim(adapter_r1="illumina", adapter_r2="illumina")
    assert (both.adapter_r1, both.adapter_r2) == (adapter_trim.TRUSEQ_R1, adapter_trim.TRUSEQ_R2)
    assert adapter_trim.TRUSEQ_R1 == "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
    assert adapter_trim.TRUSEQ_R2 == "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"
    for bad in (dict(min_overlap=7), dict(max_diff=-1), dict(diff_percent=101), dict(min_adapter=65),
                dict(adapter_r1="ACGU" * 4), dict(adapter_r2="ACG")):
        with pytest.raises(ValueError, match="AdapterTrim.%s" % list(bad)[0]):
            AdapterTrim(**bad)
    with pytest.raises(ValueError, match="nothing to do"):
        AdapterTrim(overlap=False)


def test_need_adapter_trim():
    s = AdapterTrim(min_overlap=20)
    assert need_adapter_trim(None) is None and need_adapter_trim(s) is s
    for bad in (True, False, "illumina", 4, {}, (True, "", "", 30, 5, 20, 10), AdapterTrim, ReadFilter()):
        with pytest.raises(ValueError, match="adapter_trim"):
            need_adapter_trim(bad)


def test_totals_as_counters():
    assert adapter_trim.adapter_totals_counters(TOTALS) == COUNTED
    assert list(adapter_trim.adapter_totals_counters(TOTALS)) == list(ADAPTER_COUNTER_KEYS)
    assert ADAPTER_COUNTER_KEYS == ("adapter_reads_cut", "adapter_bases_cut", "adapter_cut_by_overlap",
                                    "adapter_cut_by_sequence", "adapter_overlapping_pairs")


def test_the_keyword_is_keyword_only_on_every_route():
    assert len(ALL_ROUTES) == 12
    for fn in ALL_ROUTES:
        p = inspect.signature(fn).parameters["adapter_trim"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn.__name__
        assert "read_filter" in inspect.signature(fn).parameters


def test_the_file_level_scans_check_the_keyword_before_any_file_is_opened():
    pair, single = ("no.fa", "no.csv", "r1.fq", "r2.fq"), ("no.fa", "no.csv", "r1.fq")
    for call, files in ((scan.scan_pair_end_files, pair), (scan.scan_pair_end_report, pair),
                        (scan.scan_single_end_files, single), (scan.scan_single_end_report, single),
                        (multi_csv_scan.scan_report, pair), (multi_csv_scan.scan_report, single),
                        (multi_csv_scan.scan_report, ("no.fa", "no.txt", "r1.fq", "r2.fq")),
                        (multi_csv_scan.scan_multi_csv_report, ("no.fa", "no.txt", "r1.fq", "r2.fq"))):
        with pytest.raises(ValueError, match="adapter_trim"):
            call(*files, adapter_trim="illumina")
        with pytest.raises(ValueError, match="adapter_trim"):
            call(*files, adapter_trim=True)
    # single-end input is trimmed by sequence: without adapter_r1 there is nothing to look for
    for call, files in ((scan.scan_single_end_files, single), (scan.scan_single_end_report, single),
                        (multi_csv_scan.scan_report, single),
                        (multi_csv_scan.scan_multi_csv_report, ("no.fa", "no.txt", "r1.fq"))):
        with pytest.raises(ValueError, match="adapter_trim.*adapter_r1"):
            call(*files, adapter_trim=AdapterTrim(adapter_r2="illumina"))


# ---- the counters -----------------------------------------------------------------------------------------------------

class _Totals:
    """A totals tensor as far as ``scan.trimmed_reads`` and ``scan.filtered_reads`` look."""

    def __init__(self, values):
        self.values = values

    def cpu(self):
        return self

    def tolist(self):
        return list(self.values)


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_counters_keys_and_order(route, monkeypatch):
    """With the trimming alone, with both keywords, with neither."""
    _, (count_key, tot, chunks), front, back = route
    found = [b"a", b"drop", b"b"]
    calls = []

    def trim(ix, config, *batches):
        calls.append(("trim", ix, config, batches))
        return tuple("cut " + b for b in batches) + (_Totals(TOTALS),)

    def filt(ix, config, *batches):
        calls.append(("filter", ix, config, batches))
        return tuple("kept " + b for b in batches) + (_Totals(RF_TOTALS),)
    monkeypatch.setattr(adapter_trim, "trim_adapters_device", trim)
    monkeypatch.setattr(read_filter, "filter_reads_device", filt)
    at, rf = AdapterTrim(), ReadFilter()

    def counters_with(adapter, quality):
        del calls[:]
        kept, trimmed = scan.trimmed_reads("ix", adapter, "l", "r")
        kept, counted = scan.filtered_reads("ix", quality, *kept)
        produced = counted(trimmed((found, *scan.route_counters(count_key, 150, len(found), tot, chunks))))
        return kept, scan.finish_matches(produced[0], _Mapper(), 50, False, *produced[1:])[1]
    kept, counters = counters_with(at, None)
    assert kept == ("cut l", "cut r") and calls == [("trim", "ix", at, ("l", "r"))]
    assert list(counters) == front + list(ADAPTER_COUNTER_KEYS) + FILTER_KEYS + back
    assert {k: counters[k] for k in ADAPTER_COUNTER_KEYS} == COUNTED and counters[count_key] == 150
    kept, counters = counters_with(at, rf)
    assert kept == ("kept cut l", "kept cut r")
    assert calls == [("trim", "ix", at, ("l", "r")), ("filter", "ix", rf, ("cut l", "cut r"))]
    assert list(counters) == front + list(ADAPTER_COUNTER_KEYS) + list(COUNTER_KEYS) + FILTER_KEYS + back
    assert {k: counters[k] for k in COUNTER_KEYS} == RF_COUNTED
    # with neither: nothing is called, the batches are the same objects, the counters exactly today's
    kept, counters = counters_with(None, None)
    assert kept == ("l", "r") and calls == []
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
            tot = dict(TOT, **{("pairs" if kind == "pair" else "reads"): 10},
                       **(COUNTED if "adapter_trim" in kw else {}), **(RF_COUNTED if "read_filter" in kw else {}))
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
    at, rf = AdapterTrim(adapter_r1="illumina"), ReadFilter()
    _, counters = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", chunk_bytes=4096, adapter_trim=at)
    assert seen[-1] == ("pair", {"max_read_len": None, "adapter_trim": at})
    assert list(counters) == PAIR_FRONT + list(ADAPTER_COUNTER_KEYS) + FILTER_KEYS + ["chunks"]
    assert counters["pairs"] == 20 and counters["adapter_reads_cut"] == 2 * COUNTED["adapter_reads_cut"]   # summed
    _, counters = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", chunk_bytes=4096, adapter_trim=at,
                                           read_filter=rf)
    assert seen[-1] == ("pair", {"max_read_len": None, "read_filter": rf, "adapter_trim": at})
    assert list(counters) == PAIR_FRONT + list(ADAPTER_COUNTER_KEYS) + list(COUNTER_KEYS) + FILTER_KEYS + ["chunks"]
    _, counters = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", chunk_bytes=4096)
    assert seen[-1] == ("pair", {"max_read_len": None})
    assert list(counters) == PAIR_FRONT + FILTER_KEYS + ["chunks"]
    _, counters = scan.scan_single_end_files("ref.fa", "x.csv", "a.fq", chunk_bytes=4096, adapter_trim=at)
    assert seen[-1] == ("single", {"max_read_len": None, "adapter_trim": at})
    assert list(counters) == ["reads", "matches_before_filtering"] + list(ADAPTER_COUNTER_KEYS) + FILTER_KEYS + \
        ["retried_reads", "chunks"]
    scan.scan_single_end_files("ref.fa", "x.csv", "a.fq", chunk_bytes=4096, originals=True)
    assert seen[-1] == ("single", {"max_read_len": None, "originals": True})


def test_whole_file_routes_cut_trim_filter_scan(monkeypatch):
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

    def trimmed(ix, config, *batches):
        calls.append(("trim", config, batches))
        return tuple(_Batch("trimmed " + b) for b in batches) + (_Totals(TOTALS),)

    def filtered(ix, config, *batches):
        calls.append(("filter", config, batches))
        return tuple(_Batch("kept " + b) for b in batches) + (_Totals(RF_TOTALS),)

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
    monkeypatch.setattr(adapter_trim, "trim_adapters_device", trimmed)
    monkeypatch.setattr(read_filter, "filter_reads_device", filtered)
    monkeypatch.setattr(scan, "pairs_found", pairs_found)
    monkeypatch.setattr(scan, "single_end_found", single("device"))
    monkeypatch.setattr(scan, "_single_end_host_found", single("host"))
    at, rf = AdapterTrim(adapter_r1="illumina"), ReadFilter(poly_g_min=0)
    _, counters = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", adapter_trim=at)
    assert calls == [("trim", at, ("cut a.fq", "cut b.fq")), ("pairs", ["trimmed cut a.fq", "trimmed cut b.fq"])]
    assert {k: counters[k] for k in ADAPTER_COUNTER_KEYS} == COUNTED and not set(COUNTER_KEYS) & set(counters)
    del calls[:]
    _, counters = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", adapter_trim=at, read_filter=rf)
    assert calls == [("trim", at, ("cut a.fq", "cut b.fq")), ("filter", rf, ("trimmed cut a.fq", "trimmed cut b.fq")),
                     ("pairs", ["kept trimmed cut a.fq", "kept trimmed cut b.fq"])]
    assert list(counters)[:len(PAIR_FRONT) + 12] == PAIR_FRONT + list(ADAPTER_COUNTER_KEYS) + list(COUNTER_KEYS)
    del calls[:]
    scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq")
    assert calls == [("pairs", ["cut a.fq", "cut b.fq"])]
    for route in ("device", "host"):
        del calls[:]
        _, counters = scan.scan_single_end_files("ref.fa", "x.csv", "a.fq", route=route, adapter_trim=at, read_filter=rf)
        assert calls == [("trim", at, ("cut a.fq",)), ("filter", rf, ("trimmed cut a.fq",)),
                         (route, ["kept trimmed cut a.fq"])]
        assert {k: counters[k] for k in ADAPTER_COUNTER_KEYS} == COUNTED
        del calls[:]
        _, counters = scan.scan_single_end_files("ref.fa", "x.csv", "a.fq", route=route)
        assert calls == [(route, ["cut a.fq"])] and not set(ADAPTER_COUNTER_KEYS) & set(counters)


def test_the_streamed_pair_route_asks_for_the_full_cut_only_with_a_keyword(monkeypatch):
    seen = []

    def source_stream(indexer, sources, chunk_bytes, max_read_len, names, scan_records=None, lean=None, **kw):
        seen.append((lean, kw))
        return iter(())
    monkeypatch.setattr(scan_stream, "_scan_source_stream", source_stream)
    at, rf = AdapterTrim(adapter_r1="illumina"), ReadFilter()
    scan_stream.scan_pair_source_stream("ix", "r1", "r2", 4096)
    scan_stream.scan_pair_source_stream("ix", "r1", "r2", 4096, adapter_trim=at)
    scan_stream.scan_pair_source_stream("ix", "r1", "r2", 4096, adapter_trim=at, read_filter=rf)
    scan_stream.scan_single_text_stream("ix", "r1", 4096)
    scan_stream.scan_single_text_stream("ix", "r1", 4096, adapter_trim=at)
    assert seen == [(None, {}), (False, {"adapter_trim": at}), (False, {"read_filter": rf, "adapter_trim": at}),
                    (None, {}), (None, {"adapter_trim": at})]


def test_a_chunk_is_cut_the_full_way_trimmed_filtered_then_scanned(monkeypatch):
    from genefuserust_amd import fastq
    calls = []

    class _B:
        n_records, n_newlines = 3, 12

        def __init__(self, name):
            self.name = name

    monkeypatch.setattr(fastq, "fastq_cut_device", lambda ix, t, lean=False: (calls.append(("cut", t, lean)), _B(t))[1])
    monkeypatch.setattr(scan_stream, "_record_cuts", lambda batches, texts, final, names: (3, [3] * len(texts), [0] * len(texts)))

    def trim_chunk(ix, config, batches, m):
        calls.append(("trim", config, [b.name for b in batches], m))
        return [_B("trimmed " + b.name) for b in batches], _Totals(TOTALS)

    def filter_chunk(ix, config, batches, m):
        calls.append(("filter", config, [b.name for b in batches], m))
        return ["kept " + b.name for b in batches], _Totals(RF_TOTALS)
    monkeypatch.setattr(scan_stream, "_trim_chunk", trim_chunk)
    monkeypatch.setattr(scan_stream, "_filter_chunk", filter_chunk)

    def scan_records(ix, texts, batches, m, done, max_read_len, names):
        calls.append(("scan", [b if isinstance(b, str) else b.name for b in batches]))
        return ("rec", b"", b"", [], {"pairs": m})
    at, rf = AdapterTrim(), ReadFilter()
    args = ("ix", ["a", "b"], ["t1", "t2"], [False, False], 0, None, True)
    _, _, (out, m, last) = scan_stream._scan_chunk(*args, scan_records, adapter_trim=at)
    assert calls == [("cut", "t1", False), ("cut", "t2", False), ("trim", at, ["t1", "t2"], 3),
                     ("scan", ["trimmed t1", "trimmed t2"])]
    assert out[4] == dict({"pairs": 3}, **COUNTED) and list(out[4]) == ["pairs"] + list(ADAPTER_COUNTER_KEYS)
    del calls[:]
    _, _, (out, m, last) = scan_stream._scan_chunk(*args, scan_records, lean=True, read_filter=rf, adapter_trim=at)
    assert calls == [("cut", "t1", False), ("cut", "t2", False), ("trim", at, ["t1", "t2"], 3),
                     ("filter", rf, ["trimmed t1", "trimmed t2"], 3), ("scan", ["kept trimmed t1", "kept trimmed t2"])]
    assert list(out[4]) == ["pairs"] + list(ADAPTER_COUNTER_KEYS) + list(COUNTER_KEYS)
    # K indexes: every one's totals gain the same counts
    many = lambda *a: [("rec", b"", b"", [], {"pairs": 3}), ("rec", b"", b"", [], {"pairs": 3})]   # noqa: E731
    _, _, (out, _, _) = scan_stream._scan_chunk(*args, many, adapter_trim=at)
    assert [o[4] for o in out] == [dict({"pairs": 3}, **COUNTED)] * 2
    # without: today's call, the lean cut for pairs, nothing in between
    del calls[:]
    _, _, (out, _, _) = scan_stream._scan_chunk(*args, scan_records)
    assert calls == [("cut", "t1", True), ("cut", "t2", True), ("scan", ["t1", "t2"])] and out[4] == {"pairs": 3}


def test_scan_report_hands_the_keyword_on_only_when_set(monkeypatch):
    seen = []
    monkeypatch.setattr(scan, "scan_pair_end_report", lambda *a, **k: (seen.append(("pair", k)), ([], {}))[1])
    monkeypatch.setattr(scan, "scan_single_end_report", lambda *a, **k: (seen.append(("single", k)), ([], {}))[1])
    monkeypatch.setattr(multi_csv_scan, "scan_multi_csv_report", lambda *a, **k: (seen.append(("multi", k)), [])[1])
    at = AdapterTrim(adapter_r1="illumina")
    for files in (("ref.fa", "x.csv", "r1.fq", "r2.fq"), ("ref.fa", "x.csv", "r1.fq"), ("ref.fa", "list.txt", "r1.fq", "r2.fq")):
        multi_csv_scan.scan_report(*files, adapter_trim=at)
        multi_csv_scan.scan_report(*files)
    assert [w for w, _ in seen] == ["pair", "pair", "single", "single", "multi", "multi"]
    assert [k.get("adapter_trim", "absent") for _, k in seen] == [at, "absent"] * 3
    assert all("read_filter" not in k for _, k in seen)


def test_multi_csv_streamed_hands_the_keyword_on_only_when_set(monkeypatch):
    seen = []

    def source_stream(ix, sources, chunk_bytes, max_read_len, names, scan_records=None, lean=None, **kw):
        seen.append((lean, kw))
        tot = dict(TOT, pairs=4, **(COUNTED if "adapter_trim" in kw else {}), **(RF_COUNTED if "read_filter" in kw else {}))
        yield [("rec", b"", b"", [], dict(tot)), ("rec", b"", b"", [], dict(tot))]
        yield [("rec", b"", b"", [], dict(tot)), ("rec", b"", b"", [], dict(tot))]
    monkeypatch.setattr(scan_stream, "_scan_source_stream", source_stream)
    monkeypatch.setattr(scan_stream, "open_fastq_sources", lambda opened, files, inflate="host": list(files))
    import genefuserust_amd.fusion_mapper as fusion_mapper
    import genefuserust_amd.read_pair as read_pair
    monkeypatch.setattr(fusion_mapper, "FusionMapper", lambda ix: _Mapper())
    monkeypatch.setattr(read_pair, "finish_pair_hits", lambda *a: [])
    monkeypatch.setattr(scan, "named_from_device", lambda hits, rec, names, *orig: [])
    at, rf = AdapterTrim(), ReadFilter()
    out = multi_csv_scan._stream_multi_csv(["ix0", "ix1"], ("a.fq", "b.fq"), 4096, adapter_trim=at)
    assert seen[-1] == (False, {"adapter_trim": at})
    for _, before, after in out:   # every CSV reports the same totals, summed over the chunks
        assert list(before) == PAIR_FRONT + list(ADAPTER_COUNTER_KEYS)
        assert {k: before[k] for k in ADAPTER_COUNTER_KEYS} == {k: 2 * v for k, v in COUNTED.items()}
        assert after == {"chunks": 2}
    out = multi_csv_scan._stream_multi_csv(["ix0", "ix1"], ("a.fq", "b.fq"), 4096, adapter_trim=at, read_filter=rf)
    assert seen[-1] == (False, {"read_filter": rf, "adapter_trim": at})
    assert [list(before) for _, before, _ in out] == [PAIR_FRONT + list(ADAPTER_COUNTER_KEYS) + list(COUNTER_KEYS)] * 2
    out = multi_csv_scan._stream_multi_csv(["ix0", "ix1"], ("a.fq", "b.fq"), 4096)
    assert seen[-1] == (False, {})
    assert [list(before) for _, before, _ in out] == [PAIR_FRONT] * 2


# ---- the command line -------------------------------------------------------------------------------------------------

def test_the_command_line_options_reach_scan_report(monkeypatch, tmp_path, capsys):
    from genefuserust_amd import cli
    base = ["-1", "a.fq", "-f", "x.csv", "-r", "ref.fa"]
    a = cli.parser().parse_args(base)
    assert a.trim_adapters is False and all(getattr(a, k) is None for k in cli.ADAPTER_TRIM_OPTIONS)
    assert cli._adapter_trim(a) is None and cli._read_filter(a) is None
    assert not set(cli.ADAPTER_TRIM_OPTIONS) & set(cli.READ_FILTER_OPTIONS)          # a group of their own
    assert cli._adapter_trim(cli.parser().parse_args(base + ["--trim-adapters"])) == AdapterTrim()
    options = {"--adapter-r1": ("adapter_r1", "illumina"), "--adapter-r2": ("adapter_r2", "ACGTACGTACGTAA"),
               "--adapter-min-overlap": ("min_overlap", 20), "--adapter-max-diff": ("max_diff", 2),
               "--adapter-diff-percent": ("diff_percent", 10), "--adapter-min-match": ("min_adapter", 12)}
    assert sorted(f for f, _ in options.values()) + ["overlap"] == sorted(f.name for f in dataclasses.fields(AdapterTrim))
    for option, (field, value) in options.items():   # each sets its field, and implies the switch
        got = cli._adapter_trim(cli.parser().parse_args(base + [option, str(value)]))
        assert got == AdapterTrim(**{field: value}) and cli._read_filter(cli.parser().parse_args(base + [option, str(value)])) is None
    every = [x for option, (_, value) in options.items() for x in (option, str(value))]
    assert cli._adapter_trim(cli.parser().parse_args(base + every + ["--trim-adapters"])) == \
        AdapterTrim(**{f: v for f, v in options.values()})
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
    assert cli.main(files + csv) == 0 and "adapter_trim" not in seen[-1][1]                # off: the call of today
    assert cli.main(files + csv + ["--trim-adapters"]) == 0 and seen[-1][1]["adapter_trim"] == AdapterTrim()
    assert "read_filter" not in seen[-1][1]
    assert cli.main(files + csv + ["--adapter-r1", "illumina", "--read-filter"]) == 0
    assert seen[-1][1]["adapter_trim"] == AdapterTrim(adapter_r1="illumina") and seen[-1][1]["read_filter"] == ReadFilter()
    assert cli.main(files + lst + ["--trim-adapters", "--adapter-max-diff", "3"]) == 0
    assert seen[-1] == ("one", dict(seen[-1][1], adapter_trim=AdapterTrim(max_diff=3)))
    assert cli.main(files + lst + ["--chunk-bytes", "4096", "--adapter-min-overlap", "25"]) == 0
    assert seen[-1][0] == "streamed list" and seen[-1][1]["adapter_trim"] == AdapterTrim(min_overlap=25)
    assert cli.main(files + lst + ["--chunk-bytes", "4096"]) == 0 and "adapter_trim" not in seen[-1][1]
    capsys.readouterr()
    # a value out of range ends the run with a message, before the scan
    count = len(seen)
    assert cli.main(files + csv + ["--adapter-min-overlap", "7"]) == 1 and len(seen) == count
    assert "ERROR: AdapterTrim.min_overlap" in capsys.readouterr().err
    assert cli.main(files + csv + ["--adapter-r2", "ACGN" * 4]) == 1 and len(seen) == count
    assert "ERROR: AdapterTrim.adapter_r2" in capsys.readouterr().err
