"""The UMI step off the device: ``Umi`` and ``need_umi`` refuse what the header refuses, the command line builds the
``Umi`` its options ask for, the totals become the five counters and the ``umi`` object of the QC report, every route
takes ``umi`` — and hands nothing new down when it is None."""
import inspect
import json
from contextlib import contextmanager

import pytest

from genefuserust_amd import cli, multi_csv_scan, read_qc, scan, scan_stream, umi
from genefuserust_amd.adapter_trim import ADAPTER_COUNTER_KEYS, AdapterTrim
from genefuserust_amd.dedup import DEDUP_COUNTER_KEYS, Dedup
from genefuserust_amd.read_filter import COUNTER_KEYS, ReadFilter
from genefuserust_amd.umi import UMI_COUNTER_KEYS, Umi, need_umi, umi_totals_counters
from tests import umi_model as model

TOT = {"merged_pairs": 1, "retried_reads": 2}


def test_umi_refuses_what_the_header_refuses():
    u = Umi()
    assert (u.source, u.length, u.skip, u.inline) == ("name", 0, 0, False)
    for source in ("read1", "read2", "per_read"):
        for length in (1, 8, 32):
            for skip in (0, 1, 32):
                u = Umi(source, length, skip)
                assert u.inline and model.settings_ok(umi.SOURCES[source], length, skip)
                s = u.settings()
                assert (s.source, s.length, s.skip) == (model.SOURCES[source], length, skip)
    assert Umi("per_read", 8).describe() == {"source": "per_read", "length": 8, "skip": 0}
    bad = [("name", 8, 0), ("name", 0, 1), ("read1", 0, 0), ("read1", 33, 0), ("read2", 8, -1), ("per_read", 8, 33),
           ("read1", -1, 0), ("index1", 8, 0), ("READ1", 8, 0), (1, 8, 0), (None, 0, 0), ("read1", 8.0, 0),
           ("read1", True, 0), ("read1", 8, None), ("read1", "8", 0)]
    for args in bad:
        with pytest.raises(ValueError, match="Umi"):
            Umi(*args)
    with pytest.raises(ValueError, match="Umi"):
        Umi("read1")          # an inline source needs a length
    assert umi.SOURCES == model.SOURCES and (umi.MAX_LEN, umi.MAX_SKIP, umi.MAX_FIELD, umi.TOTALS) == \
        (model.MAX_LEN, model.MAX_SKIP, model.MAX_FIELD, model.TOTALS)
    # read2 needs pairs; per_read does not
    with pytest.raises(ValueError, match="read2"):
        Umi("read2", 8).need_sides(1)
    assert Umi("read2", 8).need_sides(2) and Umi("per_read", 8).need_sides(1) and Umi().need_sides(1)


def test_need_umi():
    u = Umi("read1", 8, 2)
    assert need_umi(None) is None and need_umi(u) is u
    for bad in ("read1", True, 8, {"source": "name"}, Umi):
        with pytest.raises(ValueError, match="umi must be None or a Umi"):
            need_umi(bad)


def test_totals_counters():
    assert UMI_COUNTER_KEYS == ("umi_reads_tagged", "umi_missing", "umi_with_n", "umi_bases_cut", "umi_too_short")
    assert umi_totals_counters([100, 90, 4, 3, 1800, 6, 55]) == dict(zip(UMI_COUNTER_KEYS, (90, 4, 3, 1800, 6)))
    q = b"F" * 12
    got = model.cut(model.PER_READ, 8, 2, [((b"ACGTACNTAAGG", q), (b"ACGTACGTAAGG", q)), ((b"ACGT", q[:4]), (b"ACGTACGTAAGG", q))])
    assert umi_totals_counters(got.totals) == dict(zip(UMI_COUNTER_KEYS, (1, 0, 1, 20, 1))) and got.totals[6] == 16


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


def test_every_route_that_takes_dedup_takes_umi_keyword_only():
    routes = _routes()
    # the public routes, by name; whatever else takes the two keywords (helpers, later routes) is held to the same
    named = {(fn.__module__.rsplit(".", 1)[-1], fn.__name__) for fn in routes}
    assert named >= {("scan", "scan_pair_end_files"), ("scan", "scan_pair_end_report"),
                     ("scan", "scan_single_end_files"), ("scan", "scan_single_end_report"),
                     ("multi_csv_scan", "scan_multi_csv_report"), ("multi_csv_scan", "scan_report"),
                     ("scan_stream", "scan_pair_source_stream"), ("scan_stream", "scan_single_text_stream")}
    for fn in routes:
        assert "dedup" in inspect.signature(fn).parameters, fn.__name__
        p = inspect.signature(fn).parameters["umi"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn.__name__
    p = inspect.signature(Dedup.apply).parameters["umi_codes"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None


def test_the_file_level_scans_check_the_keyword_before_any_file_is_opened():
    pair, single = ("no.fa", "no.csv", "r1.fq", "r2.fq"), ("no.fa", "no.csv", "r1.fq")
    calls = ((scan.scan_pair_end_files, pair), (scan.scan_pair_end_report, pair),
             (scan.scan_single_end_files, single), (scan.scan_single_end_report, single),
             (multi_csv_scan.scan_report, pair), (multi_csv_scan.scan_report, single),
             (multi_csv_scan.scan_report, ("no.fa", "no.txt", "r1.fq", "r2.fq")),
             (multi_csv_scan.scan_multi_csv_report, ("no.fa", "no.txt", "r1.fq", "r2.fq")))
    for call, files in calls:
        for bad in ("read1", True):
            with pytest.raises(ValueError, match="umi must be None or a Umi"):
                call(*files, umi=bad)
    for call in (scan_stream.scan_pair_source_stream, scan_stream.scan_single_text_stream):
        with pytest.raises(ValueError, match="umi must be None or a Umi"):
            call("ix", *(("r1", "r2") if call is scan_stream.scan_pair_source_stream else ("r1",)), umi="name")
        # ... also when another step is set
        for other in ({"read_filter": ReadFilter()}, {"adapter_trim": AdapterTrim()}, {"qc": read_qc.ReadQc()},
                      {"dedup": Dedup()}):
            with pytest.raises(ValueError, match="umi must be None or a Umi"):
                call("ix", *(("r1", "r2") if call is scan_stream.scan_pair_source_stream else ("r1",)), umi="name",
                     **other)
    # read2 with single-end input
    for call, files in calls:
        if len(files) == 3:
            with pytest.raises(ValueError, match="read2"):
                call(*files, umi=Umi("read2", 8))
    with pytest.raises(ValueError, match="read2"):
        multi_csv_scan.scan_multi_csv_report("no.fa", "no.txt", "r1.fq", umi=Umi("read2", 8))
    with pytest.raises(ValueError, match="read2"):
        scan_stream.scan_single_text_stream("ix", "r1", umi=Umi("read2", 8))


# ---- the routes hand the keyword on only when it is set -----------------------------------------------------------------

class _Totals:
    def __init__(self, values):
        self.values = list(values)

    def cpu(self):
        return self

    def tolist(self):
        return self.values


class _Dedup(Dedup):
    """A collector that only writes down what it is offered — with today's signature: no ``umi_codes``."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def apply(self, indexer, *batches, stream=None):
        self.calls.append(batches)
        return tuple(batches), _Totals([5, 5, 3, 2, 300, 0])


class _Keyed(_Dedup):
    def apply(self, indexer, *batches, stream=None, umi_codes=None):
        self.calls.append((batches, umi_codes))
        return tuple(batches), _Totals([5, 5, 3, 2, 300, 0])


class _Bases:
    device = "cpu"


class _Batch(str):
    bases = _Bases()

    def max_read_len(self):
        return 7


class _Indexer:
    m_fusion_seq = ()

    def close(self):
        pass


class _Mapper:
    m_indexer = None

    def filter_matches(self, found, threshold):
        return found, {"complexity": 0}

    def sort_matches(self, kept):
        return kept


@contextmanager
def _open_index(*a, **k):
    yield _Indexer(), []


def test_streamed_routes_hand_the_keyword_on_only_when_set(monkeypatch):
    seen = []

    def stream(kind):
        def run(ix, *args, **kw):   # today's signature: whatever is not handed on is not there
            seen.append((kind, kw))
            tot = dict(TOT, **{("pairs" if kind == "pair" else "reads"): 10})
            if "umi" in kw:
                tot.update(dict(zip(UMI_COUNTER_KEYS, (9, 0, 1, 180, 1))))
            yield "rec", b"", b"", [], tot
        return run
    monkeypatch.setattr(scan, "open_index", _open_index)
    monkeypatch.setattr(scan, "FusionMapper", lambda ix: _Mapper())
    monkeypatch.setattr(scan, "finish_pair_hits", lambda *a: [])
    monkeypatch.setattr(scan, "named_from_device", lambda hits, rec, names, *orig: [])
    monkeypatch.setattr(scan_stream, "open_fastq_sources", lambda opened, files, inflate="host": list(files))
    monkeypatch.setattr(scan_stream, "scan_pair_source_stream", stream("pair"))
    monkeypatch.setattr(scan_stream, "scan_single_text_stream", stream("single"))
    u = Umi("per_read", 8, 2)
    _, with_umi = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", chunk_bytes=4096, umi=u)
    assert seen[-1] == ("pair", {"max_read_len": None, "umi": u})
    _, without = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", chunk_bytes=4096)
    assert seen[-1] == ("pair", {"max_read_len": None})
    keys = list(with_umi)
    at = keys.index("umi_reads_tagged")
    assert tuple(keys[at:at + 5]) == UMI_COUNTER_KEYS and keys[:at] + keys[at + 5:] == list(without)
    assert {k: with_umi[k] for k in UMI_COUNTER_KEYS} == dict(zip(UMI_COUNTER_KEYS, (9, 0, 1, 180, 1)))
    scan.scan_single_end_report("ref.fa", "x.csv", "a.fq", chunk_bytes=4096, umi=Umi())
    assert seen[-1][0] == "single" and set(seen[-1][1]) == {"max_read_len", "umi"}
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

    def cut(ix, config, *batches, stream=None):
        calls.append(("umi", config.source, batches))
        return tuple(_Batch("tagged " + b) for b in batches) + ("codes", _Totals([5, 4, 0, 1, 80, 1, 9]))

    def named(ix, text, batch, stream=None):
        calls.append(("names", bytes(text.numpy()), batch))
        return "name codes", _Totals([5, 4, 1, 0, 0, 0, 0])

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
    monkeypatch.setattr(umi, "cut_umis_device", cut)
    monkeypatch.setattr(umi, "name_umis_device", named)
    monkeypatch.setattr(scan, "pairs_found", found("pairs", "pairs"))
    monkeypatch.setattr(scan, "single_end_found", found("device", "reads"))
    monkeypatch.setattr(scan, "_single_end_host_found", found("host", "reads"))


def test_whole_file_routes_tag_first_and_count_in_front_of_the_trimming(monkeypatch):
    calls = []
    _whole_file_stubs(monkeypatch, calls)
    d, cfg, trim, u = _Keyed(), ReadFilter(), AdapterTrim(), Umi("per_read", 8, 2)
    qc = read_qc.ReadQc()
    qc.measure = lambda ix, stage, *b, stream=None: calls.append((stage, b))
    _, counters = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", read_filter=cfg, adapter_trim=trim,
                                           dedup=d, qc=qc, umi=u)
    tagged = ("tagged cut a.fq", "tagged cut b.fq")
    kept = tuple("kept cut-to-insert " + t for t in tagged)
    # QC "before" on the raw records, then the UMIs, the trimming, the filter, the removal with the codes, QC "after"
    assert calls == [("before", ("cut a.fq", "cut b.fq")), ("umi", "per_read", ("cut a.fq", "cut b.fq")),
                     ("trim", tagged), ("filter", tuple("cut-to-insert " + t for t in tagged)), ("after", kept), ("pairs",)]
    assert d.calls == [(kept, "codes")]
    keys = list(counters)
    at = keys.index(UMI_COUNTER_KEYS[0])
    assert tuple(keys[at:at + 21]) == UMI_COUNTER_KEYS + ADAPTER_COUNTER_KEYS + COUNTER_KEYS + DEDUP_COUNTER_KEYS
    assert [counters[k] for k in UMI_COUNTER_KEYS] == [4, 0, 1, 80, 1]
    # alone: it cuts, "after" is measured, and the other counters are today's
    del calls[:]
    _, alone = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", umi=u, qc=qc)
    assert calls == [("before", ("cut a.fq", "cut b.fq")), ("umi", "per_read", ("cut a.fq", "cut b.fq")),
                     ("after", tagged), ("pairs",)]
    # the name source alone moves no byte: R1's text goes up for the names, and "after" is not measured; with the
    # removal behind it, it is
    raw = ("cut a.fq", "cut b.fq")
    del calls[:]
    scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", umi=Umi(), qc=qc)
    assert calls == [("before", raw), ("names", b"text", "cut a.fq"), ("pairs",)]
    del calls[:], d.calls[:]
    scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", umi=Umi(), qc=qc, dedup=d)
    assert calls == [("before", raw), ("names", b"text", "cut a.fq"), ("after", raw), ("pairs",)]
    assert d.calls == [(raw, "name codes")]
    for route in ("device", "host"):
        del calls[:]
        scan.scan_single_end_files("ref.fa", "x.csv", "a.fq", route=route, umi=Umi(), qc=qc)
        assert calls == [("before", ("cut a.fq",)), ("names", b"text", "cut a.fq"), (route,)]
        del calls[:]
        scan.scan_single_end_files("ref.fa", "x.csv", "a.fq", route=route, umi=Umi("read1", 4), qc=qc)
        assert calls == [("before", ("cut a.fq",)), ("umi", "read1", ("cut a.fq",)), ("after", ("tagged cut a.fq",)),
                         (route,)]
    _, plain = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq")
    keys = list(alone)
    at = keys.index("umi_reads_tagged")
    assert tuple(keys[at:at + 5]) == UMI_COUNTER_KEYS and keys[:at] + keys[at + 5:] == list(plain)
    # umi=None: a Dedup with today's signature is called as today, and nothing is tagged
    for route in ("device", "host"):
        old = _Dedup()
        del calls[:]
        scan.scan_single_end_files("ref.fa", "x.csv", "a.fq", route=route, dedup=old)
        assert calls == [(route,)] and old.calls == [("cut a.fq",)]
        del calls[:], d.calls[:]
        scan.scan_single_end_files("ref.fa", "x.csv", "a.fq", route=route, dedup=d, umi=Umi("read1", 4))
        assert calls == [("umi", "read1", ("cut a.fq",)), (route,)] and d.calls == [(("tagged cut a.fq",), "codes")]


def test_the_streamed_routes_ask_for_the_full_cut_only_with_an_inline_source(monkeypatch):
    seen = []

    def source_stream(indexer, sources, chunk_bytes, max_read_len, names, scan_records=None, lean=None, **kw):
        seen.append((lean, kw))
        return iter(())
    monkeypatch.setattr(scan_stream, "_scan_source_stream", source_stream)
    cut, name = Umi("read1", 8), Umi()
    scan_stream.scan_pair_source_stream("ix", "r1", "r2", 4096)
    scan_stream.scan_pair_source_stream("ix", "r1", "r2", 4096, umi=cut)
    scan_stream.scan_pair_source_stream("ix", "r1", "r2", 4096, umi=name)
    scan_stream.scan_single_text_stream("ix", "r1", 4096)
    scan_stream.scan_single_text_stream("ix", "r1", 4096, umi=cut)
    assert seen == [(None, {}), (False, {"umi": cut}), (None, {"umi": name}), (None, {}), (None, {"umi": cut})]


class _B:
    """A batch of 5 records as far as ``_scan_chunk`` looks."""
    n_records, n_newlines = 5, 20

    def __init__(self, name, offsets=(0, 1, 2, 3, 4, 5)):
        self.name, self.offsets = name, list(offsets)

    def _replace(self, **kw):
        out = _B(self.name, kw.get("offsets", self.offsets))
        out.n_records = kw["n_records"]
        return out


def test_a_chunk_tags_the_records_it_scans_never_the_ones_it_carries_over(monkeypatch):
    """``_scan_chunk``: an inline source takes the full cut whatever ``lean`` says, the name source leaves it; the first
    m = 3 of a batch's 5 records are tagged, ahead of the filter; the codes go to the removal; the totals stand in
    front of the filter's, for one index and for a list of them."""
    from genefuserust_amd import fastq
    calls = []
    monkeypatch.setattr(fastq, "fastq_cut_device", lambda ix, t, lean=False: (calls.append(("cut", t, lean)), _B(t))[1])
    monkeypatch.setattr(scan_stream, "_record_cuts",
                        lambda batches, texts, final, names: (3, [5] * len(texts), [0] * len(texts)))

    def filter_chunk(ix, config, batches, m):
        calls.append(("filter", [b.name for b in batches], m))
        return [_B("kept " + b.name, b.offsets[:m + 1]) for b in batches], _Totals([0] * 8)

    def cut_umis(ix, config, *batches, stream=None):
        calls.append(("umi", [(b.name, b.n_records, len(b.offsets)) for b in batches]))
        return tuple(_B("tagged " + b.name, b.offsets) for b in batches) + ("codes", _Totals([3, 2, 0, 0, 40, 1, 7]))

    def name_umis(ix, text, batch, stream=None):
        calls.append(("names", text, batch.name, batch.n_records))
        return "name codes", _Totals([3, 2, 1, 0, 0, 0, 0])
    monkeypatch.setattr(scan_stream, "_filter_chunk", filter_chunk)
    monkeypatch.setattr(umi, "cut_umis_device", cut_umis)
    monkeypatch.setattr(umi, "name_umis_device", name_umis)

    class _Chunks(_Keyed):
        def apply(self, indexer, *batches, stream=None, umi_codes=None):
            calls.append(("dedup", [b.name for b in batches], umi_codes))
            return tuple(_B("unique " + b.name, b.offsets) for b in batches), _Totals([3, 3, 2, 1, 150, 0])

    def scan_records(ix, texts, batches, m, done, max_read_len, names):
        calls.append(("scan", [b.name for b in batches], m))
        return ("rec", b"", b"", [], {"pairs": m})
    d = _Chunks()
    out = scan_stream._scan_chunk("ix", ["r1", "r2"], ["t1", "t2"], [False, False], 0, None, True, scan_records, True,
                                  read_filter=ReadFilter(), dedup=d, umi=Umi("per_read", 8, 2))
    assert calls == [("cut", "t1", False), ("cut", "t2", False), ("umi", [("t1", 3, 4), ("t2", 3, 4)]),
                     ("filter", ["tagged t1", "tagged t2"], 3), ("dedup", ["kept tagged t1", "kept tagged t2"], "codes"),
                     ("scan", ["unique kept tagged t1", "unique kept tagged t2"], 3)]
    tot = out[2][0][4]
    assert list(tot) == ["pairs"] + list(UMI_COUNTER_KEYS) + list(COUNTER_KEYS) + list(DEDUP_COUNTER_KEYS)
    assert [tot[k] for k in UMI_COUNTER_KEYS] == [2, 0, 0, 40, 1]
    # the name source alone: the lean cut stays, R1's text is read, the batches go on as they are; a list of indexes
    del calls[:]
    out = scan_stream._scan_chunk("ix", ["r1", "r2"], ["t1", "t2"], [False, False], 0, None, True,
                                  lambda *a: [scan_records(*a), scan_records(*a)], True, umi=Umi())
    assert calls == [("cut", "t1", True), ("cut", "t2", True), ("names", "t1", "t1", 3), ("scan", ["t1", "t2"], 3),
                     ("scan", ["t1", "t2"], 3)]
    assert [list(per_index[4]) for per_index in out[2][0]] == [["pairs"] + list(UMI_COUNTER_KEYS)] * 2
    # ... with dedup: the codes of the names
    del calls[:]
    scan_stream._scan_chunk("ix", ["r1"], ["t1"], [False], 0, None, True, scan_records, None, dedup=d, umi=Umi())
    assert calls == [("cut", "t1", False), ("names", "t1", "t1", 3), ("dedup", ["t1"], "name codes"),
                     ("scan", ["unique t1"], 3)]
    # qc with the name source alone: the full cut, "before", and no "after" -- no byte has moved, as on the whole-file
    # routes; with an inline source alone "after" is measured on the cut records; with the removal behind the names too
    qc = read_qc.ReadQc()
    qc.measure = lambda ix, stage, *b, stream=None: calls.append((stage, [(x.name, x.n_records) for x in b]))
    raw = [("t1", 3), ("t2", 3)]
    del calls[:]
    scan_stream._scan_chunk("ix", ["r1", "r2"], ["t1", "t2"], [False, False], 0, None, True, scan_records, True,
                            qc=qc, umi=Umi())
    assert calls == [("cut", "t1", False), ("cut", "t2", False), ("before", raw), ("names", "t1", "t1", 3),
                     ("scan", ["t1", "t2"], 3)]
    del calls[:]
    scan_stream._scan_chunk("ix", ["r1", "r2"], ["t1", "t2"], [False, False], 0, None, True, scan_records, True,
                            qc=qc, umi=Umi("read2", 8))
    assert calls == [("cut", "t1", False), ("cut", "t2", False), ("before", raw),
                     ("umi", [("t1", 3, 4), ("t2", 3, 4)]), ("after", [("tagged t1", 3), ("tagged t2", 3)]),
                     ("scan", ["tagged t1", "tagged t2"], 3)]
    del calls[:]
    scan_stream._scan_chunk("ix", ["r1"], ["t1"], [False], 0, None, True, scan_records, None, qc=qc, dedup=d, umi=Umi())
    assert calls == [("cut", "t1", False), ("before", [("t1", 3)]), ("names", "t1", "t1", 3),
                     ("dedup", ["t1"], "name codes"), ("after", [("unique t1", 3)]), ("scan", ["unique t1"], 3)]
    # without it: the cut and the scan of today
    del calls[:]
    scan_stream._scan_chunk("ix", ["r1", "r2"], ["t1", "t2"], [False, False], 0, None, True, scan_records, True)
    assert calls == [("cut", "t1", True), ("cut", "t2", True), ("scan", ["t1", "t2"], 3)]


def test_multi_csv_hands_the_keyword_on_only_when_set(monkeypatch):
    calls = []
    monkeypatch.setattr(multi_csv_scan, "scan_multi_csv_report", lambda *a, **kw: calls.append(kw) or [])
    u = Umi("read1", 6)
    multi_csv_scan.scan_report("ref.fa", "list.txt", "a.fq", "b.fq", umi=u)
    multi_csv_scan.scan_report("ref.fa", "list.txt", "a.fq", "b.fq")
    assert calls[0]["umi"] is u and "umi" not in calls[1]
    seen = []
    from genefuserust_amd import scan as scan_module
    monkeypatch.setattr(scan_module, "scan_pair_end_report", lambda *a, **kw: seen.append(kw) or ([], {}))
    multi_csv_scan.scan_report("ref.fa", "x.csv", "a.fq", "b.fq", umi=u)
    multi_csv_scan.scan_report("ref.fa", "x.csv", "a.fq", "b.fq")
    assert seen[0]["umi"] is u and "umi" not in seen[1]


# ---- the command line ---------------------------------------------------------------------------------------------------

def _args(*extra):
    return cli.parser().parse_args(["-1", "a.fq", "-f", "x.csv", "-r", "ref.fa", *extra])


def test_cli_options():
    assert cli._umi(_args()) is None
    u = cli._umi(_args("--umi-loc", "name"))
    assert isinstance(u, Umi) and (u.source, u.length, u.skip) == ("name", 0, 0)
    u = cli._umi(_args("--umi-loc", "per_read", "--umi-len", "8", "--umi-skip", "2"))
    assert (u.source, u.length, u.skip) == ("per_read", 8, 2)
    u = cli._umi(_args("--umi-loc", "read2", "--umi-len", "12"))
    assert (u.source, u.length, u.skip) == ("read2", 12, 0)
    for lonely in (("--umi-len", "8"), ("--umi-skip", "2"), ("--umi-len", "8", "--umi-skip", "0")):
        with pytest.raises(ValueError, match="needs --umi-loc"):
            cli._umi(_args(*lonely))
    for bad in (("--umi-loc", "read1"), ("--umi-loc", "read1", "--umi-len", "33"), ("--umi-loc", "name", "--umi-len", "8"),
                ("--umi-loc", "read1", "--umi-len", "8", "--umi-skip", "40")):
        with pytest.raises(ValueError, match="Umi"):
            cli._umi(_args(*bad))
    with pytest.raises(SystemExit):
        _args("--umi-loc", "index1")
    text = cli.parser().format_help()
    for option in ("--umi-loc", "--umi-len", "--umi-skip", "per_read"):
        assert option in text


def test_cli_hands_the_umi_to_the_scan_and_to_the_qc_report(monkeypatch, tmp_path):
    seen = []

    def scan_report(ref, fusion, r1, r2, **kw):
        seen.append(kw)
        counters = {"pairs": 0}
        if "umi" in kw:
            counters.update(dict(zip(UMI_COUNTER_KEYS, (7, 0, 1, 140, 2))))
        return [], counters
    monkeypatch.setattr(multi_csv_scan, "scan_report", scan_report)
    files = []
    for name in ("a.fq", "x.csv", "ref.fa"):
        (tmp_path / name).write_text("")
        files.append(str(tmp_path / name))
    base = ["-1", files[0], "-f", files[1], "-r", files[2], "-h", "", "-j", ""]
    assert cli.main(base) == 0 and "umi" not in seen[-1]
    assert cli.main(base + ["--umi-loc", "per_read", "--umi-len", "8", "--umi-skip", "2"]) == 0
    assert isinstance(seen[-1]["umi"], Umi) and seen[-1]["umi"].describe() == {"source": "per_read", "length": 8, "skip": 2}
    assert cli.main(base + ["--umi-len", "8"]) == 1 and cli.main(base + ["--umi-loc", "read1"]) == 1
    qc_file = tmp_path / "qc.json"
    assert cli.main(base + ["--umi-loc", "per_read", "--umi-len", "8", "--umi-skip", "2", "--qc-json", str(qc_file)]) == 0
    doc = json.loads(qc_file.read_text())
    assert doc["umi"] == {"source": "per_read", "length": 8, "skip": 2, "tagged_reads": 7, "reads_without_umi": 0,
                          "umis_with_N": 1, "cut_bases": 140, "too_short_reads": 2}
    assert cli.main(base + ["--qc-json", str(qc_file)]) == 0 and "umi" not in json.loads(qc_file.read_text())


def test_report_document_adds_the_umi_object_with_the_counters():
    class _Result:
        def summary(self, stage):
            return {}

        def insert_size(self):
            return None

        def tables(self, stage):
            return ()
    counters = dict(zip(UMI_COUNTER_KEYS, (90, 4, 3, 0, 0)))
    doc = read_qc.report_document(_Result(), counters, umi=Umi())
    assert doc["umi"] == {"source": "name", "length": 0, "skip": 0, "tagged_reads": 90, "reads_without_umi": 4,
                          "umis_with_N": 3, "cut_bases": 0, "too_short_reads": 0}
    assert list(doc) == ["summary", "umi"]
    assert "umi" not in read_qc.report_document(_Result(), {"pairs": 1}, umi=Umi())
    assert "umi" not in read_qc.report_document(_Result())
    assert list(read_qc.report_document(_Result(), counters)["umi"])[0] == "tagged_reads"
