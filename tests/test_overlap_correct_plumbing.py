"""The overlap correction off the device: every route that takes ``adapter_trim`` takes ``overlap_correct`` — keyword
only, refused for a wrong type and for single-end input before a file is opened, and handed down only when it is set;
the chain calls the step behind the UMI step and ahead of the trimming, feeds its output onwards, forces the full cut
and measures QC "after"; the five counters stand between the UMI step's and the trimming's; the command line builds the
``OverlapCorrect`` its options ask for; the QC report gains ``overlap_correction``."""
import inspect
import json
from contextlib import contextmanager

import pytest

from genefuserust_amd import cli, multi_csv_scan, overlap_correct, read_qc, scan, scan_stream, umi
from genefuserust_amd.adapter_trim import ADAPTER_COUNTER_KEYS, AdapterTrim
from genefuserust_amd.dedup import DEDUP_COUNTER_KEYS, Dedup
from genefuserust_amd.overlap_correct import CORRECT_COUNTER_KEYS, OverlapCorrect
from genefuserust_amd.read_filter import COUNTER_KEYS, ReadFilter
from genefuserust_amd.umi import UMI_COUNTER_KEYS, Umi

TOT = {"merged_pairs": 1, "retried_reads": 2}
REFUSED = "overlap_correct must be None or an OverlapCorrect"


def _routes():
    """Every function of the three route modules that takes ``adapter_trim``."""
    out = []
    for module in (scan, scan_stream, multi_csv_scan):
        for name, fn in vars(module).items():
            if inspect.isfunction(fn) and fn.__module__ == module.__name__:
                if "adapter_trim" in inspect.signature(fn).parameters and fn.__name__ not in ("trimmed_reads", "_trim_chunk"):
                    out.append(fn)
    return out


def test_every_route_that_takes_adapter_trim_takes_the_keyword_keyword_only():
    routes = _routes()
    named = {(fn.__module__.rsplit(".", 1)[-1], fn.__name__) for fn in routes}
    assert named >= {("scan", "scan_pair_end_files"), ("scan", "scan_pair_end_report"),
                     ("scan", "scan_single_end_files"), ("scan", "scan_single_end_report"), ("scan", "streamed_found"),
                     ("multi_csv_scan", "scan_multi_csv_report"), ("multi_csv_scan", "scan_report"),
                     ("scan_stream", "scan_pair_source_stream"), ("scan_stream", "scan_single_text_stream"),
                     ("scan_stream", "_scan_chunk"), ("scan_stream", "_scan_source_stream")}
    for fn in routes:
        p = inspect.signature(fn).parameters["overlap_correct"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn.__name__


def test_the_file_level_scans_check_the_keyword_before_any_file_is_opened():
    pair, single = ("no.fa", "no.csv", "r1.fq", "r2.fq"), ("no.fa", "no.csv", "r1.fq")
    calls = ((scan.scan_pair_end_files, pair), (scan.scan_pair_end_report, pair),
             (scan.scan_single_end_files, single), (scan.scan_single_end_report, single),
             (multi_csv_scan.scan_report, pair), (multi_csv_scan.scan_report, single),
             (multi_csv_scan.scan_report, ("no.fa", "no.txt", "r1.fq", "r2.fq")),
             (multi_csv_scan.scan_multi_csv_report, ("no.fa", "no.txt", "r1.fq", "r2.fq")),
             (multi_csv_scan.scan_multi_csv_report, ("no.fa", "no.txt", "r1.fq")))
    for call, files in calls:
        for bad in ("on", True, AdapterTrim(), OverlapCorrect):
            with pytest.raises(ValueError, match=REFUSED):
                call(*files, overlap_correct=bad)
            with pytest.raises(ValueError, match=REFUSED):
                call(*files, overlap_correct=bad, chunk_bytes=4096)
    for call in (scan_stream.scan_pair_source_stream, scan_stream.scan_single_text_stream):
        sources = ("r1", "r2") if call is scan_stream.scan_pair_source_stream else ("r1",)
        with pytest.raises(ValueError, match=REFUSED):
            call("ix", *sources, overlap_correct=1)
        for other in ({"read_filter": ReadFilter()}, {"adapter_trim": AdapterTrim(adapter_r1="illumina")},
                      {"qc": read_qc.ReadQc()}, {"dedup": Dedup()}, {"umi": Umi()}):
            with pytest.raises(ValueError, match=REFUSED):
                call("ix", *sources, overlap_correct=1, **other)
    # single-end input: the correction needs pairs -- the single-end branch of multi-CSV mode too
    for call, files in calls:
        if len(files) == 3:
            for more in ({}, {"chunk_bytes": 4096}):
                with pytest.raises(ValueError, match="needs pairs"):
                    call(*files, overlap_correct=OverlapCorrect(), **more)
    with pytest.raises(ValueError, match="needs pairs"):
        scan_stream.scan_single_text_stream("ix", "r1", overlap_correct=OverlapCorrect())
    with pytest.raises(ValueError, match="needs pairs"):
        multi_csv_scan.scan_report("no.fa", "no.txt", "r1.fq", overlap_correct=OverlapCorrect())


# ---- the routes hand the keyword on only when it is set -----------------------------------------------------------------

class _Totals:
    def __init__(self, values):
        self.values = list(values)

    def cpu(self):
        return self

    def tolist(self):
        return self.values


class _Keyed(Dedup):
    def __init__(self):
        super().__init__()
        self.calls = []

    def apply(self, indexer, *batches, stream=None, umi_codes=None):
        self.calls.append((batches, umi_codes))
        return tuple(batches), _Totals([5, 5, 3, 2, 300, 0])


class _Bases:
    device = "cpu"


class _Batch(str):
    bases = _Bases()
    quals = offsets = property(str)   # (which batch they are of)

    def max_read_len(self):
        return 7


class _Indexer:
    m_fusion_seq = ()

    def close(self):
        pass


class _Mapper:
    m_indexer = None

    def __init__(self, ix=None):
        pass

    def filter_matches(self, found, threshold):
        return found, {"complexity": 0}

    @staticmethod
    def sort_matches(kept):
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
            if "overlap_correct" in kw:
                tot.update(dict(zip(CORRECT_COUNTER_KEYS, (8, 4, 5, 6, 2))))
            if "adapter_trim" in kw:
                tot.update(dict.fromkeys(ADAPTER_COUNTER_KEYS, 1))
            yield "rec", b"", b"", [], tot
        return run
    monkeypatch.setattr(scan, "open_index", _open_index)
    monkeypatch.setattr(scan, "FusionMapper", lambda ix: _Mapper())
    monkeypatch.setattr(scan, "finish_pair_hits", lambda *a: [])
    monkeypatch.setattr(scan, "named_from_device", lambda hits, rec, names, *orig: [])
    monkeypatch.setattr(scan_stream, "open_fastq_sources", lambda opened, files, inflate="host": list(files))
    monkeypatch.setattr(scan_stream, "scan_pair_source_stream", stream("pair"))
    monkeypatch.setattr(scan_stream, "scan_single_text_stream", stream("single"))
    oc, u, trim = OverlapCorrect(max_diff=3), Umi("per_read", 8, 2), AdapterTrim()
    _, with_it = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", chunk_bytes=4096, overlap_correct=oc)
    assert seen[-1] == ("pair", {"max_read_len": None, "overlap_correct": oc})
    _, without = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", chunk_bytes=4096)
    assert seen[-1] == ("pair", {"max_read_len": None})
    keys = list(with_it)
    at = keys.index(CORRECT_COUNTER_KEYS[0])
    assert tuple(keys[at:at + 5]) == CORRECT_COUNTER_KEYS and keys[:at] + keys[at + 5:] == list(without)
    assert {k: with_it[k] for k in CORRECT_COUNTER_KEYS} == dict(zip(CORRECT_COUNTER_KEYS, (8, 4, 5, 6, 2)))
    # between the UMI step's and the trimming's
    _, all_three = scan.scan_pair_end_report("ref.fa", "x.csv", "a.fq", "b.fq", chunk_bytes=4096, overlap_correct=oc,
                                             umi=u, adapter_trim=trim)
    assert seen[-1] == ("pair", {"max_read_len": None, "overlap_correct": oc, "umi": u, "adapter_trim": trim})
    keys = list(all_three)
    at = keys.index(UMI_COUNTER_KEYS[0])
    assert tuple(keys[at:at + 15]) == UMI_COUNTER_KEYS + CORRECT_COUNTER_KEYS + ADAPTER_COUNTER_KEYS
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
        calls.append(("umi", batches))
        return tuple(_Batch("tagged " + b) for b in batches) + ("codes", _Totals([5, 4, 0, 1, 80, 1, 9]))

    def corrected(ix, config, batch, mate, stream=None, detail=False, inplace=False):
        calls.append(("correct", config, (batch, mate), inplace))
        return _Batch("corrected " + batch), _Batch("corrected " + mate), _Totals([5, 4, 3, 2, 7, 1])

    def found(kind, key):
        def run(*args, **kw):
            calls.append((kind,))
            return [], *scan.route_counters(key, 5, 0, TOT)
        return run
    from genefuserust_amd import adapter_trim, fastq, fusion_mapper, read_filter
    monkeypatch.setattr(scan, "FastqReaderPair", _Reader)
    monkeypatch.setattr(scan, "FastqReader", _Reader)
    monkeypatch.setattr(fastq, "FastqReaderPair", _Reader)       # (multi_csv_scan takes them from there)
    monkeypatch.setattr(fastq, "FastqReader", _Reader)
    monkeypatch.setattr(fusion_mapper, "FusionMapper", _Mapper)
    monkeypatch.setattr(multi_csv_scan, "prepare_pairs_device", lambda ix, *a: calls.append(("prepare", a[1], a[4])) or
                        type("P", (), {"max_read_len": 7})())
    monkeypatch.setattr(read_filter, "filter_reads_device", filtered)
    monkeypatch.setattr(adapter_trim, "trim_adapters_device", trimmed)
    monkeypatch.setattr(umi, "cut_umis_device", cut)
    monkeypatch.setattr(overlap_correct, "correct_overlaps_device", corrected)
    monkeypatch.setattr(scan, "pairs_found", found("pairs", "pairs"))
    monkeypatch.setattr(scan, "single_end_found", found("device", "reads"))
    monkeypatch.setattr(scan, "_single_end_host_found", found("host", "reads"))


def test_whole_file_routes_correct_behind_the_umis_and_ahead_of_the_trimming(monkeypatch):
    calls = []
    _whole_file_stubs(monkeypatch, calls)
    d, cfg, trim, u, oc = _Keyed(), ReadFilter(), AdapterTrim(), Umi("per_read", 8, 2), OverlapCorrect(good_phred=25)
    qc = read_qc.ReadQc()
    qc.measure = lambda ix, stage, *b, stream=None: calls.append((stage, b))
    _, counters = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", read_filter=cfg, adapter_trim=trim,
                                           dedup=d, qc=qc, umi=u, overlap_correct=oc)
    raw = ("cut a.fq", "cut b.fq")
    tagged = tuple("tagged " + t for t in raw)
    fixed = tuple("corrected " + t for t in tagged)
    kept = tuple("kept cut-to-insert " + t for t in fixed)
    # QC "before", the UMIs, the correction (not in place), the trimming on its output, the filter, the removal, QC "after"
    assert calls == [("before", raw), ("umi", raw), ("correct", oc, tagged, False), ("trim", fixed),
                     ("filter", tuple("cut-to-insert " + t for t in fixed)), ("after", kept), ("pairs",)]
    assert d.calls == [(kept, "codes")]
    keys = list(counters)
    at = keys.index(UMI_COUNTER_KEYS[0])
    assert tuple(keys[at:at + 26]) == (UMI_COUNTER_KEYS + CORRECT_COUNTER_KEYS + ADAPTER_COUNTER_KEYS + COUNTER_KEYS
                                       + DEDUP_COUNTER_KEYS)
    assert [counters[k] for k in CORRECT_COUNTER_KEYS] == [4, 3, 2, 7, 1]
    # alone: it counts as a step for QC "after", and the other counters are today's
    del calls[:]
    _, alone = scan.scan_pair_end_report("ref.fa", "x.csv", "a.fq", "b.fq", overlap_correct=oc, qc=qc)
    assert calls == [("before", raw), ("correct", oc, raw, False), ("after", tuple("corrected " + t for t in raw)),
                     ("pairs",)]
    _, plain = scan.scan_pair_end_report("ref.fa", "x.csv", "a.fq", "b.fq")
    keys = list(alone)
    at = keys.index(CORRECT_COUNTER_KEYS[0])
    assert tuple(keys[at:at + 5]) == CORRECT_COUNTER_KEYS and keys[:at] + keys[at + 5:] == list(plain)
    # None: the step function is not called, and the chain is today's
    del calls[:]
    monkeypatch.setattr(scan, "corrected_reads", None)
    scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", adapter_trim=trim, qc=qc)
    assert calls == [("before", raw), ("trim", raw), ("after", tuple("cut-to-insert " + t for t in raw)), ("pairs",)]


def test_multi_csv_whole_file_mode_corrects_once(monkeypatch, tmp_path):
    calls = []
    _whole_file_stubs(monkeypatch, calls)
    monkeypatch.setattr(multi_csv_scan, "read_csv_list", lambda f: ["one.csv", "two.csv"])
    monkeypatch.setattr(multi_csv_scan, "scan_prepared_pairs_device", lambda *a, **k: None)
    monkeypatch.setattr(scan, "read_contigs", lambda f: {})
    oc, trim = OverlapCorrect(), AdapterTrim()
    out = multi_csv_scan.scan_multi_csv_report("ref.fa", "list.txt", "a.fq", "b.fq", overlap_correct=oc, adapter_trim=trim)
    raw = ("cut a.fq", "cut b.fq")
    fixed = tuple("corrected " + t for t in raw)
    trimmed = tuple("cut-to-insert " + t for t in fixed)
    # once for the list: the correction, the trimming on its output, the pairs prepared from that, then a scan per CSV
    assert calls == [("correct", oc, raw, False), ("trim", fixed), ("prepare", *trimmed), ("pairs",), ("pairs",)]
    for _, _, counters in out:
        keys = list(counters)
        at = keys.index(CORRECT_COUNTER_KEYS[0])
        assert tuple(keys[at:at + 10]) == CORRECT_COUNTER_KEYS + ADAPTER_COUNTER_KEYS
        assert [counters[k] for k in CORRECT_COUNTER_KEYS] == [4, 3, 2, 7, 1]


def test_the_streamed_routes_ask_for_the_full_cut(monkeypatch):
    seen = []

    def source_stream(indexer, sources, chunk_bytes, max_read_len, names, scan_records=None, lean=None, **kw):
        seen.append((lean, kw))
        return iter(())
    monkeypatch.setattr(scan_stream, "_scan_source_stream", source_stream)
    oc = OverlapCorrect()
    scan_stream.scan_pair_source_stream("ix", "r1", "r2", 4096)
    scan_stream.scan_pair_source_stream("ix", "r1", "r2", 4096, overlap_correct=oc)
    scan_stream.scan_single_text_stream("ix", "r1", 4096)
    assert seen == [(None, {}), (False, {"overlap_correct": oc}), (None, {})]


class _B:
    """A batch of 5 records as far as ``_scan_chunk`` looks."""
    n_records, n_newlines = 5, 20

    def __init__(self, name, offsets=(0, 1, 2, 3, 4, 5)):
        self.name, self.offsets = name, list(offsets)

    def _replace(self, **kw):
        out = _B(self.name, kw.get("offsets", self.offsets))
        out.n_records = kw["n_records"]
        return out


def test_a_chunk_corrects_the_pairs_it_scans_never_the_ones_it_carries_over(monkeypatch):
    """``_scan_chunk``: the keyword takes the full cut whatever ``lean`` says; the first m = 3 of a batch's 5 pairs are
    corrected, behind the UMI step and ahead of the trimming, which gets its output; "after" is measured; the totals
    stand between the UMI step's and the trimming's, for one index and for a list of them."""
    from genefuserust_amd import fastq
    calls = []
    monkeypatch.setattr(fastq, "fastq_cut_device", lambda ix, t, lean=False: (calls.append(("cut", t, lean)), _B(t))[1])
    monkeypatch.setattr(scan_stream, "_record_cuts",
                        lambda batches, texts, final, names: (3, [5] * len(texts), [0] * len(texts)))

    def trim_chunk(ix, config, batches, m):
        calls.append(("trim", [b.name for b in batches], m))
        return [_B("trimmed " + b.name, b.offsets[:m + 1]) for b in batches], _Totals([0] * 6)

    def cut_umis(ix, config, *batches, stream=None):
        calls.append(("umi", [(b.name, b.n_records, len(b.offsets)) for b in batches]))
        return tuple(_B("tagged " + b.name, b.offsets) for b in batches) + ("codes", _Totals([3, 2, 0, 0, 40, 1, 7]))

    def correct(ix, config, batch, mate, stream=None, detail=False, inplace=False):
        calls.append(("correct", [(b.name, b.n_records, len(b.offsets)) for b in (batch, mate)], inplace))
        return _B("corrected " + batch.name, batch.offsets), _B("corrected " + mate.name, mate.offsets), \
            _Totals([3, 3, 2, 2, 5, 1])
    monkeypatch.setattr(scan_stream, "_trim_chunk", trim_chunk)
    monkeypatch.setattr(umi, "cut_umis_device", cut_umis)
    monkeypatch.setattr(overlap_correct, "correct_overlaps_device", correct)

    def scan_records(ix, texts, batches, m, done, max_read_len, names):
        calls.append(("scan", [b.name for b in batches], m))
        return ("rec", b"", b"", [], {"pairs": m})
    qc = read_qc.ReadQc()
    qc.measure = lambda ix, stage, *b, stream=None: calls.append((stage, [x.name for x in b]))
    oc = OverlapCorrect()
    out = scan_stream._scan_chunk("ix", ["r1", "r2"], ["t1", "t2"], [False, False], 0, None, True, scan_records, True,
                                  adapter_trim=AdapterTrim(), umi=Umi("per_read", 8, 2), overlap_correct=oc, qc=qc)
    assert calls == [("cut", "t1", False), ("cut", "t2", False), ("before", ["t1", "t2"]),
                     ("umi", [("t1", 3, 4), ("t2", 3, 4)]),
                     ("correct", [("tagged t1", 3, 4), ("tagged t2", 3, 4)], False),
                     ("trim", ["corrected tagged t1", "corrected tagged t2"], 3),
                     ("after", ["trimmed corrected tagged t1", "trimmed corrected tagged t2"]),
                     ("scan", ["trimmed corrected tagged t1", "trimmed corrected tagged t2"], 3)]
    tot = out[2][0][4]
    assert list(tot) == ["pairs"] + list(UMI_COUNTER_KEYS) + list(CORRECT_COUNTER_KEYS) + list(ADAPTER_COUNTER_KEYS)
    assert [tot[k] for k in CORRECT_COUNTER_KEYS] == [3, 2, 2, 5, 1]
    # alone: the full cut though lean was asked for, the pairs scanned are the corrected ones; a list of indexes; with
    # qc "after" is measured, for the keyword counts as a step
    del calls[:]
    out = scan_stream._scan_chunk("ix", ["r1", "r2"], ["t1", "t2"], [False, False], 0, None, True,
                                  lambda *a: [scan_records(*a), scan_records(*a)], True, overlap_correct=oc)
    assert calls == [("cut", "t1", False), ("cut", "t2", False), ("correct", [("t1", 3, 4), ("t2", 3, 4)], False),
                     ("scan", ["corrected t1", "corrected t2"], 3), ("scan", ["corrected t1", "corrected t2"], 3)]
    assert [list(per_index[4]) for per_index in out[2][0]] == [["pairs"] + list(CORRECT_COUNTER_KEYS)] * 2
    del calls[:]
    scan_stream._scan_chunk("ix", ["r1", "r2"], ["t1", "t2"], [False, False], 0, None, True, scan_records, None,
                            overlap_correct=oc, qc=qc)
    assert calls == [("cut", "t1", False), ("cut", "t2", False), ("before", ["t1", "t2"]),
                     ("correct", [("t1", 3, 4), ("t2", 3, 4)], False), ("after", ["corrected t1", "corrected t2"]),
                     ("scan", ["corrected t1", "corrected t2"], 3)]
    # without it: the cut and the scan of today
    del calls[:]
    scan_stream._scan_chunk("ix", ["r1", "r2"], ["t1", "t2"], [False, False], 0, None, True, scan_records, True)
    assert calls == [("cut", "t1", True), ("cut", "t2", True), ("scan", ["t1", "t2"], 3)]


def test_multi_csv_hands_the_keyword_on_only_when_set(monkeypatch):
    calls = []
    monkeypatch.setattr(multi_csv_scan, "scan_multi_csv_report", lambda *a, **kw: calls.append(kw) or [])
    oc = OverlapCorrect(min_overlap=20)
    multi_csv_scan.scan_report("ref.fa", "list.txt", "a.fq", "b.fq", overlap_correct=oc)
    multi_csv_scan.scan_report("ref.fa", "list.txt", "a.fq", "b.fq")
    assert calls[0]["overlap_correct"] is oc and "overlap_correct" not in calls[1]
    seen = []
    monkeypatch.setattr(scan, "scan_pair_end_report", lambda *a, **kw: seen.append(kw) or ([], {}))
    multi_csv_scan.scan_report("ref.fa", "x.csv", "a.fq", "b.fq", overlap_correct=oc)
    multi_csv_scan.scan_report("ref.fa", "x.csv", "a.fq", "b.fq")
    assert seen[0]["overlap_correct"] is oc and "overlap_correct" not in seen[1]


def test_the_streamed_multi_csv_scan_hands_the_keyword_to_the_chunk_loop(monkeypatch):
    seen = []

    def source_stream(indexer, sources, chunk_bytes, max_read_len, names, scan_records=None, lean=None, **kw):
        seen.append((lean, kw))
        return iter(())
    monkeypatch.setattr(scan_stream, "_scan_source_stream", source_stream)
    monkeypatch.setattr(scan_stream, "open_fastq_sources", lambda opened, files, inflate="host": list(files))
    from genefuserust_amd import fusion_mapper
    monkeypatch.setattr(fusion_mapper, "FusionMapper", _Mapper)
    oc = OverlapCorrect()
    out = multi_csv_scan._stream_multi_csv(["ix0", "ix1"], ("a.fq", "b.fq"), 4096, overlap_correct=oc)
    assert seen[-1] == (False, {"overlap_correct": oc})
    for _, before, _ in out:
        assert tuple(k for k in before if k in CORRECT_COUNTER_KEYS) == CORRECT_COUNTER_KEYS
    multi_csv_scan._stream_multi_csv(["ix0"], ("a.fq", "b.fq"), 4096)
    assert seen[-1] == (False, {})


# ---- the command line ---------------------------------------------------------------------------------------------------

def _args(*extra, pair=True):
    return cli.parser().parse_args(["-1", "a.fq", *(["-2", "b.fq"] if pair else []), "-f", "x.csv", "-r", "ref.fa", *extra])


def test_cli_options():
    assert cli._overlap_correct(_args()) is None and cli._overlap_correct(_args(pair=False)) is None
    assert cli._overlap_correct(_args("--correct-overlap")) == OverlapCorrect()
    # each of the five implies it
    assert cli._overlap_correct(_args("--correct-min-overlap", "12")) == OverlapCorrect(min_overlap=12)
    assert cli._overlap_correct(_args("--correct-max-diff", "2")) == OverlapCorrect(max_diff=2)
    assert cli._overlap_correct(_args("--correct-diff-percent", "10")) == OverlapCorrect(diff_percent=10)
    assert cli._overlap_correct(_args("--correct-good-phred", "25")) == OverlapCorrect(good_phred=25)
    assert cli._overlap_correct(_args("--correct-bad-phred", "5")) == OverlapCorrect(bad_phred=5)
    assert cli._overlap_correct(_args("--correct-overlap", "--correct-good-phred", "20", "--correct-bad-phred", "10")) == \
        OverlapCorrect(good_phred=20, bad_phred=10)
    for bad in (("--correct-min-overlap", "7"), ("--correct-bad-phred", "30"), ("--correct-good-phred", "94"),
                ("--correct-diff-percent", "101"), ("--correct-max-diff=-1",)):
        with pytest.raises(ValueError, match="OverlapCorrect"):
            cli._overlap_correct(_args(*bad))
    # with -1 alone it is an error
    for lonely in (("--correct-overlap",), ("--correct-max-diff", "2")):
        with pytest.raises(ValueError, match="needs pairs"):
            cli._overlap_correct(_args(*lonely, pair=False))
    text = cli.parser().format_help()
    for option in ("--correct-overlap", "--correct-min-overlap", "--correct-max-diff", "--correct-diff-percent",
                   "--correct-good-phred", "--correct-bad-phred"):
        assert option in text


def test_cli_hands_the_keyword_to_the_scan_and_the_counters_to_the_qc_report(monkeypatch, tmp_path):
    seen = []

    def scan_report(ref, fusion, r1, r2, **kw):
        seen.append(kw)
        counters = {"pairs": 0}
        if "overlap_correct" in kw:
            counters.update(dict(zip(CORRECT_COUNTER_KEYS, (70, 30, 25, 41, 6))))
        return [], counters
    monkeypatch.setattr(multi_csv_scan, "scan_report", scan_report)
    files = []
    for name in ("a.fq", "b.fq", "x.csv", "ref.fa"):
        (tmp_path / name).write_text("")
        files.append(str(tmp_path / name))
    single = ["-1", files[0], "-f", files[2], "-r", files[3], "-h", "", "-j", ""]
    base = single + ["-2", files[1]]
    assert cli.main(base) == 0 and "overlap_correct" not in seen[-1]
    assert cli.main(base + ["--correct-overlap", "--correct-max-diff", "3"]) == 0
    assert seen[-1]["overlap_correct"] == OverlapCorrect(max_diff=3)
    # -1 alone, and a value out of range: an error before any work
    before = len(seen)
    assert cli.main(single + ["--correct-overlap"]) == 1 and cli.main(base + ["--correct-bad-phred", "40"]) == 1
    assert len(seen) == before
    qc_file = tmp_path / "qc.json"
    assert cli.main(base + ["--correct-overlap", "--qc-json", str(qc_file)]) == 0
    doc = json.loads(qc_file.read_text())
    assert doc["overlap_correction"] == {"overlapping_pairs": 70, "pairs_with_differences": 30, "corrected_reads": 25,
                                         "corrected_bases": 41, "differences_left": 6}
    assert cli.main(base + ["--qc-json", str(qc_file)]) == 0
    assert "overlap_correction" not in json.loads(qc_file.read_text())


def test_report_document_adds_the_object_with_the_counters():
    class _Result:
        def summary(self, stage):
            return {}

        def insert_size(self):
            return None

        def tables(self, stage):
            return ()
    counters = dict(zip(CORRECT_COUNTER_KEYS, (90, 40, 33, 50, 4)))
    doc = read_qc.report_document(_Result(), counters)
    assert doc["overlap_correction"] == {"overlapping_pairs": 90, "pairs_with_differences": 40, "corrected_reads": 33,
                                         "corrected_bases": 50, "differences_left": 4}
    assert list(doc["overlap_correction"]) == ["overlapping_pairs", "pairs_with_differences", "corrected_reads",
                                               "corrected_bases", "differences_left"]
    assert list(doc) == ["summary", "overlap_correction"]
    both = dict(counters, **dict.fromkeys(ADAPTER_COUNTER_KEYS, 1), **dict(zip(UMI_COUNTER_KEYS, (1, 1, 1, 1, 1))))
    assert list(read_qc.report_document(_Result(), both)) == ["summary", "adapter_cutting", "overlap_correction", "umi"]
    assert "overlap_correction" not in read_qc.report_document(_Result(), {"pairs": 1})
    assert "overlap_correction" not in read_qc.report_document(_Result())
