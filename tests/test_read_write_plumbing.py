"""CPU-side checks of the plumbing of ``write_reads``: what ``ReadWriter`` refuses, the counters, that every route which
takes ``dedup`` takes the keyword, checks it first, refuses it without ``chunk_bytes`` and hands nothing new down when it
is None, where the step stands in a chunk, the writer threads and their temporaries, and the command line."""
import gzip
import inspect
import os
from contextlib import contextmanager

import pytest

from genefuserust_amd import cli, multi_csv_scan, read_write, scan, scan_stream
from genefuserust_amd.dedup import DEDUP_COUNTER_KEYS, Dedup
from genefuserust_amd.read_filter import COUNTER_KEYS, ReadFilter
from genefuserust_amd.read_write import (WRITE_COUNTER_KEYS, ReadWriter, WriteResult, need_read_writer,
                                         write_totals_counters)
from genefuserust_amd.umi import UMI_COUNTER_KEYS, Umi
from tests import read_write_model as model

TOT = {"merged_pairs": 0, "retried_reads": 0, "hits": 0}


# ---- ReadWriter ---------------------------------------------------------------------------------------------------------------

def test_read_writer_refuses_what_it_cannot_write(tmp_path):
    a, b = str(tmp_path / "a.fq"), str(tmp_path / "b.fq.gz")
    w = ReadWriter(a)
    assert (w.out1, w.out2, w.umi_in_name, w.compress_level, w.outputs) == (a, None, False, 4, (a,))
    w = ReadWriter(a, b, umi_in_name=True, compress_level=9)
    assert w.outputs == (a, b) and w.umi_in_name and w.compress_level == 9
    for level in (0, 10, -1, 4.0, "4", True, None):
        with pytest.raises(ValueError, match="compress_level"):
            ReadWriter(a, compress_level=level)
    for bad in (None, "", 5, b"a.fq"):
        with pytest.raises(ValueError, match="out1"):
            ReadWriter(bad)
    with pytest.raises(ValueError, match="out2"):
        ReadWriter(a, "")
    with pytest.raises(ValueError, match="umi_in_name"):
        ReadWriter(a, umi_in_name=1)
    with pytest.raises(ValueError, match="same file"):
        ReadWriter(a, a)
    with pytest.raises(ValueError, match="same file"):
        ReadWriter(a, str(tmp_path / "sub" / ".." / "a.fq"))
    for out in ((str(tmp_path / "nowhere" / "a.fq"),), (a, str(tmp_path / "nowhere" / "b.fq"))):
        with pytest.raises(ValueError, match="does not exist"):
            ReadWriter(*out)
    assert os.listdir(tmp_path) == []      # nothing was opened


def test_need_route_refuses_before_any_file_is_opened(tmp_path):
    a, b = str(tmp_path / "a.fq"), str(tmp_path / "b.fq")
    r1, r2 = str(tmp_path / "r1.fq"), str(tmp_path / "r2.fq")
    pair, single = ReadWriter(a, b), ReadWriter(a)
    assert pair.need_route((r1, r2)) is pair and single.need_route((r1,), Umi("read1", 8)) is single
    with pytest.raises(ValueError, match="needs ReadWriter.out2"):
        single.need_route((r1, r2))
    with pytest.raises(ValueError, match="takes no ReadWriter.out2"):
        pair.need_route((r1,))
    with pytest.raises(ValueError, match="needs chunk_bytes"):
        pair.need_route((r1, r2), streamed=False)
    for inputs in ((a, r2), (r1, b), (str(tmp_path / "." / "b.fq"), r2)):
        with pytest.raises(ValueError, match="one of the inputs"):
            pair.need_route(inputs)
    tagged = ReadWriter(a, b, umi_in_name=True)
    for u in (None, Umi()):
        with pytest.raises(ValueError, match="umi_in_name needs umi with an inline source"):
            tagged.need_route((r1, r2), u)
    for u in (Umi("read1", 8), Umi("read2", 8, 2), Umi("per_read", 32)):
        assert tagged.need_route((r1, r2), u) is tagged
    assert os.listdir(tmp_path) == []


def test_need_read_writer():
    w = ReadWriter("a.fq")
    assert need_read_writer(None) is None and need_read_writer(w) is w
    for bad in ("a.fq", True, 1, ("a.fq", "b.fq"), Dedup()):
        with pytest.raises(ValueError, match="write_reads must be None or a ReadWriter"):
            need_read_writer(bad)


def test_counters():
    assert WRITE_COUNTER_KEYS == ("written_records", "written_bases", "written_bytes")
    assert write_totals_counters([90, 27000, 31000, 30500, 10]) == dict(zip(WRITE_COUNTER_KEYS, (90, 27000, 61500)))
    text = b"@a x\nACGT\n+\nFFFF\n@b\nAC\n+\nFF\n"
    want = model.format_reads([text, text], [[(b"ACG", b"FFF"), (b"AC", b"FF")], [(b"A", b"F"), (b"", b"")]])
    assert want.totals == [1, 4, 15, 11, 1] and write_totals_counters(want.totals) == model.counters(want.totals)
    assert ReadWriter("a.fq").result() == WriteResult(0, 0, (0,), 0)
    assert ReadWriter("a.fq", "b.fq").result() == WriteResult(0, 0, (0, 0), 0)
    assert read_write.capacity(100, 3) == 100 + 1 + 3 * 66


# ---- the writer threads -----------------------------------------------------------------------------------------------------

def test_files_are_written_in_order_and_renamed_at_the_end(tmp_path):
    a, b = str(tmp_path / "a.fq"), str(tmp_path / "b.fq.gz")
    w = ReadWriter(a, b, compress_level=1)
    w.open(2)
    assert sorted(os.listdir(tmp_path)) == ["a.fq.tmp", "b.fq.gz.tmp"]
    released = []
    blocks = [(b"@r%d\nACGT\n+\nFFFF\n" % k) * (k + 1) for k in range(12)]      # more blocks than the queue is deep
    for k, block in enumerate(blocks):
        w.hand_over(0, block, lambda k=k: released.append(k))
        w.hand_over(1, bytearray(block))
    w.finish()
    assert sorted(os.listdir(tmp_path)) == ["a.fq", "b.fq.gz"] and sorted(released) == list(range(12))
    assert open(a, "rb").read() == b"".join(blocks)
    packed = open(b, "rb").read()
    assert gzip.decompress(packed) == b"".join(blocks) and packed.count(b"\x1f\x8b\x08") >= 12   # a member per block
    with pytest.raises(ValueError, match="has served a scan"):
        w.open(2)
    with pytest.raises(ValueError, match="has served a scan"):
        w.need_route(("r1.fq", "r2.fq"))
    # no block at all: an empty file, and a gzip file of no bytes
    w = ReadWriter(str(tmp_path / "e.fq"), str(tmp_path / "e.fq.gz"))
    w.open(2)
    w.finish()
    assert open(w.out1, "rb").read() == b"" and gzip.decompress(open(w.out2, "rb").read()) == b""
    with pytest.raises(ValueError, match="output files for"):
        ReadWriter(str(tmp_path / "x.fq")).open(2)


def test_the_temporaries_are_removed_when_a_chunk_raises(tmp_path, monkeypatch):
    """The chunk loop with a writer: the files are opened before the first chunk, and a chunk that raises leaves
    neither the temporaries nor a thread behind; a stream that ends gives the files their names."""
    import threading

    class _Stream:
        sides = ()

        def __init__(self, *a):
            pass

        def run(self, chunk):
            for k in range(3):
                yield chunk(["t1", "t2"], [False, False])

    class _Torch:
        @staticmethod
        def device(*a):
            return "dev"

    class _Ix:
        def _handle(self):
            return 0

        def info(self):
            return {"device": 0}
    seen = []

    def scan_chunk(indexer, side_names, texts, final, done, max_read_len, names, scan_records, lean, **kw):
        w = kw["write_reads"]
        seen.append(sorted(os.listdir(tmp_path)))
        if len(seen) == fail_at:
            raise RuntimeError("chunk %d failed" % len(seen))
        w.hand_over(0, b"one %d\n" % len(seen))
        w.hand_over(1, b"two %d\n" % len(seen))
        return ("out", 1, False)
    monkeypatch.setattr(scan_stream, "ChunkStream", _Stream)
    monkeypatch.setattr(scan_stream, "_scan_chunk", scan_chunk)
    monkeypatch.setitem(__import__("sys").modules, "torch", _Torch)
    threads = threading.active_count()
    for fail_at in (2, 0):
        del seen[:]
        w = ReadWriter(str(tmp_path / "o1.fq"), str(tmp_path / "o2.fq.gz"))
        stream = scan_stream._scan_source_stream(_Ix(), ("r1", "r2"), 4096, None, True, write_reads=w)
        assert os.listdir(tmp_path) == []          # (nothing before the first chunk is asked for)
        if fail_at:
            with pytest.raises(RuntimeError, match="chunk 2 failed"):
                list(stream)
            assert seen == [["o1.fq.tmp", "o2.fq.gz.tmp"]] * 2 and os.listdir(tmp_path) == []
        else:
            assert list(stream) == ["out"] * 3
            assert sorted(os.listdir(tmp_path)) == ["o1.fq", "o2.fq.gz"]
            assert open(w.out1, "rb").read() == b"one 1\none 2\none 3\n"
            assert gzip.decompress(open(w.out2, "rb").read()) == b"two 1\ntwo 2\ntwo 3\n"
        assert threading.active_count() == threads
    # a stream that is closed early leaves nothing either
    for name in os.listdir(tmp_path):
        os.unlink(tmp_path / name)
    fail_at = 0
    w = ReadWriter(str(tmp_path / "o1.fq"), str(tmp_path / "o2.fq.gz"))
    stream = scan_stream._scan_source_stream(_Ix(), ("r1", "r2"), 4096, None, True, write_reads=w)
    assert next(stream) == "out" and len(os.listdir(tmp_path)) == 2
    stream.close()
    assert os.listdir(tmp_path) == [] and threading.active_count() == threads


def test_a_file_that_cannot_be_written_fails_the_scan_and_leaves_nothing(tmp_path):
    w = ReadWriter(str(tmp_path / "a.fq"), str(tmp_path / "b.fq"))
    w.open(2)
    w._writers[1].f.close()         # the disk is gone under R2's thread
    w.hand_over(0, b"x")
    w.hand_over(1, b"y")
    with pytest.raises(ValueError, match="closed file"):
        w.finish()
    assert os.listdir(tmp_path) == []


# ---- the routes ---------------------------------------------------------------------------------------------------------------

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


def test_every_route_that_takes_dedup_takes_write_reads_keyword_only():
    routes = _routes()
    named = {(fn.__module__.rsplit(".", 1)[-1], fn.__name__) for fn in routes}
    assert named >= {("scan", "scan_pair_end_files"), ("scan", "scan_pair_end_report"),
                     ("scan", "scan_single_end_files"), ("scan", "scan_single_end_report"),
                     ("multi_csv_scan", "scan_multi_csv_report"), ("multi_csv_scan", "scan_report"),
                     ("scan_stream", "scan_pair_source_stream"), ("scan_stream", "scan_single_text_stream"),
                     ("scan_stream", "_scan_chunk"), ("scan", "streamed_found")}
    for fn in routes:
        assert "dedup" in inspect.signature(fn).parameters, fn.__name__
        p = inspect.signature(fn).parameters["write_reads"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn.__name__


def test_the_file_level_scans_check_the_keyword_first_and_refuse_the_whole_file_routes(tmp_path):
    pair, single = ("no.fa", "no.csv", "r1.fq", "r2.fq"), ("no.fa", "no.csv", "r1.fq")
    calls = ((scan.scan_pair_end_files, pair), (scan.scan_pair_end_report, pair),
             (scan.scan_single_end_files, single), (scan.scan_single_end_report, single),
             (multi_csv_scan.scan_report, pair), (multi_csv_scan.scan_report, single),
             (multi_csv_scan.scan_report, ("no.fa", "no.txt", "r1.fq", "r2.fq")),
             (multi_csv_scan.scan_multi_csv_report, ("no.fa", "no.txt", "r1.fq", "r2.fq")))
    a, b = str(tmp_path / "a.fq"), str(tmp_path / "b.fq")
    for call, files in calls:
        for bad in ("out.fq", True):
            # ... first: in front of the other keywords' checks
            with pytest.raises(ValueError, match="write_reads must be None or a ReadWriter"):
                call(*files, write_reads=bad, umi="nonsense", dedup="nonsense")
        w = ReadWriter(a, b) if len(files) == 4 else ReadWriter(a)
        with pytest.raises(ValueError, match="write_reads needs chunk_bytes"):
            call(*files, write_reads=w)
        wrong = ReadWriter(a) if len(files) == 4 else ReadWriter(a, b)
        with pytest.raises(ValueError, match="ReadWriter.out2"):
            call(*files, write_reads=wrong, chunk_bytes=4096)
        same = ReadWriter("r1.fq", b) if len(files) == 4 else ReadWriter("r1.fq")
        with pytest.raises(ValueError, match="one of the inputs"):
            call(*files, write_reads=same, chunk_bytes=4096)
        tagged = ReadWriter(a, b, umi_in_name=True) if len(files) == 4 else ReadWriter(a, umi_in_name=True)
        for u in (None, Umi()):
            with pytest.raises(ValueError, match="umi_in_name"):
                call(*files, write_reads=tagged, chunk_bytes=4096, **({} if u is None else {"umi": u}))
    for call in (scan_stream.scan_pair_source_stream, scan_stream.scan_single_text_stream):
        sources = ("r1", "r2") if call is scan_stream.scan_pair_source_stream else ("r1",)
        with pytest.raises(ValueError, match="write_reads must be None or a ReadWriter"):
            call("ix", *sources, write_reads="out.fq", umi="nonsense")
        wrong = ReadWriter(a) if len(sources) == 2 else ReadWriter(a, b)
        with pytest.raises(ValueError, match="ReadWriter.out2"):
            call("ix", *sources, write_reads=wrong)
    assert os.listdir(tmp_path) == []


class _Mapper:
    m_indexer = None

    def filter_matches(self, found, threshold):
        return found, {"complexity": 0}

    def sort_matches(self, kept):
        return kept


class _Indexer:
    m_fusion_seq = ()

    def close(self):
        pass


@contextmanager
def _open_index(*a, **k):
    yield _Indexer(), []


def test_streamed_routes_hand_the_keyword_on_only_when_set(monkeypatch, tmp_path):
    seen = []

    def stream(kind):
        def run(ix, *args, **kw):   # today's signature: whatever is not handed on is not there
            seen.append((kind, kw))
            tot = dict(TOT, **{("pairs" if kind == "pair" else "reads"): 10})
            if "write_reads" in kw:
                tot.update(dict(zip(WRITE_COUNTER_KEYS, (9, 2700, 6100))))
            yield "rec", b"", b"", [], tot
            yield "rec", b"", b"", [], dict(tot)
        return run
    monkeypatch.setattr(scan, "open_index", _open_index)
    monkeypatch.setattr(scan, "FusionMapper", lambda ix: _Mapper())
    monkeypatch.setattr(scan, "finish_pair_hits", lambda *a: [])
    monkeypatch.setattr(scan, "named_from_device", lambda hits, rec, names, *orig: [])
    monkeypatch.setattr(scan_stream, "open_fastq_sources", lambda opened, files, inflate="host": list(files))
    monkeypatch.setattr(scan_stream, "scan_pair_source_stream", stream("pair"))
    monkeypatch.setattr(scan_stream, "scan_single_text_stream", stream("single"))
    w = ReadWriter(str(tmp_path / "a.fq"), str(tmp_path / "b.fq"))
    _, with_writer = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", chunk_bytes=4096, write_reads=w)
    assert seen[-1] == ("pair", {"max_read_len": None, "write_reads": w})
    _, without = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", chunk_bytes=4096)
    assert seen[-1] == ("pair", {"max_read_len": None})
    keys = list(with_writer)
    at = keys.index("written_records")
    assert tuple(keys[at:at + 3]) == WRITE_COUNTER_KEYS and keys[:at] + keys[at + 3:] == list(without)
    assert {k: with_writer[k] for k in WRITE_COUNTER_KEYS} == dict(zip(WRITE_COUNTER_KEYS, (18, 5400, 12200)))
    assert keys[at + 3] == "complexity"        # in front of the filter counts, as every step's
    single = ReadWriter(str(tmp_path / "a.fq"))
    scan.scan_single_end_report("ref.fa", "x.csv", "a.fq", chunk_bytes=4096, write_reads=single)
    assert seen[-1][0] == "single" and seen[-1][1] == {"max_read_len": None, "write_reads": single}
    scan.scan_single_end_report("ref.fa", "x.csv", "a.fq", chunk_bytes=4096)
    assert seen[-1] == ("single", {"max_read_len": None})


def test_the_streams_ask_for_the_full_cut_and_hand_the_writer_on_only_when_set(monkeypatch, tmp_path):
    seen = []

    def source_stream(indexer, sources, chunk_bytes, max_read_len, names, scan_records=None, lean=None, **kw):
        seen.append((lean, kw))
        return iter(())
    monkeypatch.setattr(scan_stream, "_scan_source_stream", source_stream)
    pair, single = ReadWriter(str(tmp_path / "a.fq"), str(tmp_path / "b.fq")), ReadWriter(str(tmp_path / "a.fq"))
    scan_stream.scan_pair_source_stream("ix", "r1", "r2", 4096)
    scan_stream.scan_pair_source_stream("ix", "r1", "r2", 4096, write_reads=pair)
    scan_stream.scan_single_text_stream("ix", "r1", 4096)
    scan_stream.scan_single_text_stream("ix", "r1", 4096, write_reads=single)
    assert seen == [(None, {}), (False, {"write_reads": pair}), (None, {}), (None, {"write_reads": single})]


class _Totals:
    def __init__(self, values):
        self.values = list(values)

    def cpu(self):
        return self

    def tolist(self):
        return self.values


class _B:
    """A batch of 5 records as far as ``_scan_chunk`` looks."""
    n_records, n_newlines = 5, 20

    def __init__(self, name, offsets=(0, 1, 2, 3, 4, 5)):
        self.name, self.offsets = name, list(offsets)

    def _replace(self, **kw):
        out = _B(self.name, kw.get("offsets", self.offsets))
        out.n_records = kw["n_records"]
        return out


def test_a_chunk_formats_behind_the_last_step_and_hands_over_behind_the_scan(monkeypatch, tmp_path):
    """``_scan_chunk``: the writer takes the full cut whatever ``lean`` says; the first m = 3 of a batch's 5 records are
    formatted, behind the duplicate removal and QC's "after" stage and ahead of the scan, from the chunk's texts and the
    cut's batches; the text is collected behind the scan; the totals stand behind the removal's, for one index and for
    a list of them, once."""
    from genefuserust_amd import fastq, read_qc, umi
    calls = []
    monkeypatch.setattr(fastq, "fastq_cut_device", lambda ix, t, lean=False: (calls.append(("cut", t, lean)), _B(t))[1])
    monkeypatch.setattr(scan_stream, "_record_cuts",
                        lambda batches, texts, final, names: (3, [5] * len(texts), [0] * len(texts)))

    def filter_chunk(ix, config, batches, m):
        calls.append(("filter", [b.name for b in batches], m))
        return [_B("kept " + b.name, b.offsets[:m + 1]) for b in batches], _Totals([0] * 8)

    def cut_umis(ix, config, *batches, stream=None):
        calls.append(("umi", [b.name for b in batches]))
        return tuple(_B("tagged " + b.name, b.offsets) for b in batches) + ("codes", _Totals([3, 2, 0, 0, 40, 1, 7]))
    monkeypatch.setattr(scan_stream, "_filter_chunk", filter_chunk)
    monkeypatch.setattr(umi, "cut_umis_device", cut_umis)

    class _Chunks(Dedup):
        def apply(self, indexer, *batches, stream=None, umi_codes=None):
            calls.append(("dedup", [b.name for b in batches]))
            return tuple(_B("unique " + b.name, b.offsets) for b in batches), _Totals([3, 3, 2, 1, 150, 0])

    def format_reads(indexer, texts, cuts, finals, n, pre=None, umi=None, gather=0, stream=None):
        calls.append(("format", list(texts), [b.name for b in cuts], [(b.name, b.n_records, len(b.offsets)) for b in finals],
                      n, None if pre is None else [(b.name, b.n_records) for b in pre], umi))
        return ["text"] * len(texts), ["off"] * len(texts), _Totals([2, 300, 400, 390, 1])
    monkeypatch.setattr(read_write, "format_reads_device", format_reads)

    class _Writer(ReadWriter):
        def collect(self, formatted):
            calls.append(("collect", formatted[0]))
            return write_totals_counters(formatted[2].tolist())

    def scan_records(ix, texts, batches, m, done, max_read_len, names):
        calls.append(("scan", [b.name for b in batches], m))
        return ("rec", b"", b"", [], {"pairs": m})
    qc = read_qc.ReadQc()
    qc.measure = lambda ix, stage, *b, stream=None: calls.append((stage, [x.name for x in b]))
    a, b = str(tmp_path / "a.fq"), str(tmp_path / "b.fq")
    u = Umi("per_read", 8, 2)
    out = scan_stream._scan_chunk("ix", ["r1", "r2"], ["t1", "t2"], [False, False], 0, None, True, scan_records, True,
                                  read_filter=ReadFilter(), dedup=_Chunks(), umi=u, qc=qc, write_reads=_Writer(a, b))
    final = ["unique kept tagged t1", "unique kept tagged t2"]
    assert calls == [("cut", "t1", False), ("cut", "t2", False), ("before", ["t1", "t2"]), ("umi", ["t1", "t2"]),
                     ("filter", ["tagged t1", "tagged t2"], 3), ("dedup", ["kept tagged t1", "kept tagged t2"]),
                     ("after", final),
                     ("format", ["t1", "t2"], ["t1", "t2"], [(name, 3, 4) for name in final], 3, None, None),
                     ("scan", final, 3), ("collect", ["text", "text"])]
    tot = out[2][0][4]
    assert list(tot) == ["pairs"] + list(UMI_COUNTER_KEYS) + list(COUNTER_KEYS) + list(DEDUP_COUNTER_KEYS) + \
        list(WRITE_COUNTER_KEYS)
    assert [tot[k] for k in WRITE_COUNTER_KEYS] == [2, 300, 790]
    # umi_in_name: the batches ahead of the UMI cut and the Umi go with it
    del calls[:]
    scan_stream._scan_chunk("ix", ["r1", "r2"], ["t1", "t2"], [False, False], 0, None, True, scan_records, True,
                            umi=u, write_reads=_Writer(a, b, umi_in_name=True))
    assert calls[3] == ("format", ["t1", "t2"], ["t1", "t2"], [("tagged t1", 3, 4), ("tagged t2", 3, 4)], 3,
                        [("t1", 3), ("t2", 3)], u)
    # the writer alone: the full cut, the records as they came; a list of indexes is written once
    del calls[:]
    out = scan_stream._scan_chunk("ix", ["r1"], ["t1"], [False], 0, None, True,
                                  lambda *x: [scan_records(*x), scan_records(*x)], None, write_reads=_Writer(a))
    assert calls == [("cut", "t1", False), ("format", ["t1"], ["t1"], [("t1", 3, 4)], 3, None, None), ("scan", ["t1"], 3),
                     ("scan", ["t1"], 3), ("collect", ["text"])]
    assert [list(per_index[4]) for per_index in out[2][0]] == [["pairs"] + list(WRITE_COUNTER_KEYS)] * 2
    del calls[:]
    scan_stream._scan_chunk("ix", ["r1", "r2"], ["t1", "t2"], [False, False], 0, None, True, scan_records, True,
                            write_reads=_Writer(a, b))
    assert calls[:2] == [("cut", "t1", False), ("cut", "t2", False)]      # lean is overruled
    # without it: the cut and the scan of today
    del calls[:]
    scan_stream._scan_chunk("ix", ["r1", "r2"], ["t1", "t2"], [False, False], 0, None, True, scan_records, True)
    assert calls == [("cut", "t1", True), ("cut", "t2", True), ("scan", ["t1", "t2"], 3)]
    assert os.listdir(tmp_path) == []


def test_multi_csv_hands_the_keyword_on_only_when_set(monkeypatch, tmp_path):
    calls = []
    monkeypatch.setattr(multi_csv_scan, "scan_multi_csv_report", lambda *a, **kw: calls.append(kw) or [])
    w = ReadWriter(str(tmp_path / "a.fq"), str(tmp_path / "b.fq"))
    with pytest.raises(ValueError, match="needs chunk_bytes"):      # this switch keeps a list's reads resident
        multi_csv_scan.scan_report("ref.fa", "list.txt", "a.fq", "b.fq", write_reads=w)
    multi_csv_scan.scan_report("ref.fa", "list.txt", "a.fq", "b.fq")
    assert "write_reads" not in calls[0]
    seen = []
    from genefuserust_amd import scan as scan_module
    monkeypatch.setattr(scan_module, "scan_pair_end_report", lambda *a, **kw: seen.append(kw) or ([], {}))
    multi_csv_scan.scan_report("ref.fa", "x.csv", "a.fq", "b.fq", chunk_bytes=4096, write_reads=w)
    multi_csv_scan.scan_report("ref.fa", "x.csv", "a.fq", "b.fq", chunk_bytes=4096)
    assert seen[0]["write_reads"] is w and "write_reads" not in seen[1]


# ---- the command line ---------------------------------------------------------------------------------------------------

def _args(*extra):
    return cli.parser().parse_args(["-1", "a.fq", "-f", "x.csv", "-r", "ref.fa", *extra])


def test_cli_options(tmp_path):
    assert cli._read_writer(_args()) is None
    a, b = str(tmp_path / "a.fq.gz"), str(tmp_path / "b.fq.gz")
    w = cli._read_writer(_args("--out1", a))
    assert isinstance(w, ReadWriter) and (w.out1, w.out2, w.umi_in_name, w.compress_level) == (a, None, False, 4)
    w = cli._read_writer(_args("--out1", a, "--out2", b, "--umi-in-name", "--out-compression", "7"))
    assert (w.out1, w.out2, w.umi_in_name, w.compress_level) == (a, b, True, 7)
    for lonely in (("--out2", b), ("--umi-in-name",), ("--out-compression", "3")):
        with pytest.raises(ValueError, match="needs --out1"):
            cli._read_writer(_args(*lonely))
    for bad in (("--out1", a, "--out-compression", "0"), ("--out1", a, "--out-compression", "10"), ("--out1", a, "--out2", a),
                ("--out1", str(tmp_path / "nowhere" / "a.fq"))):
        with pytest.raises(ValueError, match="ReadWriter"):
            cli._read_writer(_args(*bad))
    text = cli.parser().format_help()
    for option in ("--out1", "--out2", "--umi-in-name", "--out-compression"):
        assert option in text


def test_cli_hands_the_writer_to_a_streamed_scan(monkeypatch, tmp_path):
    seen = []
    monkeypatch.setattr(multi_csv_scan, "scan_report", lambda ref, fusion, r1, r2, **kw: seen.append(("one", kw)) or ([], {}))
    monkeypatch.setattr(multi_csv_scan, "scan_multi_csv_report",
                        lambda ref, fusion, r1, r2, **kw: seen.append(("list", kw)) or [])
    files = []
    for name in ("a.fq", "x.csv", "ref.fa", "list.txt"):
        (tmp_path / name).write_text("")
        files.append(str(tmp_path / name))
    base = ["-1", files[0], "-f", files[1], "-r", files[2], "-h", "", "-j", ""]
    out = str(tmp_path / "out.fq")
    assert cli.main(base) == 0 and "write_reads" not in seen[-1][1] and seen[-1][1]["chunk_bytes"] is None
    assert cli.main(base + ["--out1", out]) == 0
    assert isinstance(seen[-1][1]["write_reads"], ReadWriter) and seen[-1][1]["write_reads"].out1 == out
    assert seen[-1][1]["chunk_bytes"] == 128 << 20 == cli.DEFAULT_OUT_CHUNK_BYTES      # it streams, with the default
    assert cli.main(base + ["--out1", out, "--chunk-bytes", "65536"]) == 0 and seen[-1][1]["chunk_bytes"] == 65536
    assert cli.main(base + ["--out2", out]) == 1 and cli.main(base + ["--out1", out, "--out-compression", "11"]) == 1
    # a list of CSVs with --out1 goes to the streamed multi-CSV scan
    as_list = ["-1", files[0], "-f", files[3], "-r", files[2], "-h", "", "-j", ""]
    assert cli.main(as_list) == 0 and seen[-1][0] == "one"
    assert cli.main(as_list + ["--out1", out]) == 0
    assert seen[-1][0] == "list" and seen[-1][1]["chunk_bytes"] == 128 << 20 and seen[-1][1]["write_reads"].out1 == out
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")
