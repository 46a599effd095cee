"""The switch of the whole-genome alignable filter through the layers, without a GPU: ``scan.finish_matches`` with a
stub for the device call — the counters' keys and their order, the ``ValueError``s, and no call when the switch is off
— the file-level scans' checks before any file is opened, and the command line's option down to ``scan_report``."""
import inspect

import pytest

from genefuserust_amd import alignable, scan
from tests.test_scan_pieces import FILTER_KEYS, ROUTES, _Mapper


class _Match:
    def __init__(self, read: bytes):
        self.m_read = read

    def __repr__(self):
        return "match(%r)" % self.m_read


class _Indexer:
    def get_ref(self):
        return {"chr": b"the reference"}

    def info(self):
        return {"device": 3}


class _GenomeMapper(_Mapper):
    """tests/test_scan_pieces.py's stub mapper, with the index the genome filter asks for its reference and device."""
    m_indexer = _Indexer()

    def filter_matches(self, found, deletion_threshold):
        self.calls.append(("filter", deletion_threshold))
        kept = [m for m in found if m.m_read != b"drop"]
        return kept, {"complexity": len(found) - len(kept), "distance": 0, "indels": 0}


@pytest.fixture
def device_call(monkeypatch):
    """``alignable.alignable_reads_device`` replaced: reads that start with b"al" are alignable."""
    calls = []

    def stub(reference, reads, device=-1, batch_bytes=256 << 20, **kw):
        import numpy as np
        calls.append((reference, list(reads), device))
        return np.array([r.startswith(b"al") for r in reads], dtype=bool)
    monkeypatch.setattr(alignable, "alignable_reads_device", stub)
    return calls


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_counters_with_the_genome_filter_keys_and_order(route, device_call):
    _, (count_key, tot, chunks), front, back = route
    found = [_Match(b"a"), _Match(b"drop"), _Match(b"al1"), _Match(b"c"), _Match(b"al2")]
    before, after = scan.route_counters(count_key, 150, len(found), tot, chunks)
    mapper = _GenomeMapper()
    kept, counters = scan.finish_matches(found, mapper, 50, False, before, after, alignable_filter="genome")
    assert list(counters) == front + FILTER_KEYS + ["genome_alignables"] + back
    assert counters["genome_alignables"] == 2 and counters["complexity"] == 1
    assert [m.m_read for m in kept] == [b"c", b"a"]                        # (the stub's sort reverses)
    assert mapper.calls == [("filter", 50), ("sort",)]
    # one call, the reads of the matches that survived the other filters, the index's reference and device
    assert device_call == [({"chr": b"the reference"}, [b"a", b"al1", b"c", b"al2"], 3)]
    # switched off: the counters of today, and the device call is not made
    del device_call[:]
    for kw in ({}, {"alignable_filter": None}):
        kept, counters = scan.finish_matches(found, _GenomeMapper(), 50, False, before, after, **kw)
        assert list(counters) == front + FILTER_KEYS + back and len(kept) == 4
    assert device_call == []


def test_no_matches_no_call(device_call):
    kept, counters = scan.finish_matches([_Match(b"drop")], _GenomeMapper(), 50, False, {"reads": 1}, {},
                                         alignable_filter="genome")
    assert kept == [] and counters["genome_alignables"] == 0 and device_call == []


def test_the_switch_is_keyword_only_and_checked(device_call):
    assert inspect.signature(scan.finish_matches).parameters["alignable_filter"].kind is inspect.Parameter.KEYWORD_ONLY
    found = [_Match(b"a")]
    for bad in ("host", "device", True, "Genome", ""):
        with pytest.raises(ValueError, match="alignable_filter"):
            scan.finish_matches(found, _GenomeMapper(), 50, False, {}, {}, alignable_filter=bad)
    with pytest.raises(ValueError, match="remove_alignables"):
        scan.finish_matches(found, _GenomeMapper(), 50, True, {}, {}, alignable_filter="genome")
    with pytest.raises(TypeError):
        scan.finish_matches(found, _GenomeMapper(), 50, False, {}, {}, "host", "genome")
    assert device_call == []


def test_the_file_level_scans_check_the_switch_before_any_file_is_opened():
    from genefuserust_amd.multi_csv_scan import scan_report
    pair = ("no.fa", "no.csv", "r1.fq", "r2.fq")
    single = ("no.fa", "no.csv", "r1.fq")
    for call in (scan.scan_pair_end_files, scan.scan_pair_end_report):
        with pytest.raises(ValueError, match="alignable_filter"):
            call(*pair, alignable_filter="nope")
        with pytest.raises(ValueError, match="whole contigs"):
            call(*pair, alignable_filter="genome", ref_chunk_bytes=4096)
        with pytest.raises(ValueError, match="remove_alignables"):
            call(*pair, alignable_filter="genome", remove_alignables=True)
        with pytest.raises(TypeError):
            call(*pair, -1, None, None, None, "host", "host", False, False, "genome")
    for call in (scan.scan_single_end_files, scan.scan_single_end_report):
        with pytest.raises(ValueError, match="alignable_filter"):
            call(*single, alignable_filter="nope")
        with pytest.raises(ValueError, match="whole contigs"):
            call(*single, alignable_filter="genome", ref_chunk_bytes=4096)
    with pytest.raises(ValueError, match="alignable_filter"):
        scan_report(*pair, alignable_filter="nope")
    with pytest.raises(ValueError, match="whole contigs"):
        scan_report(*pair, alignable_filter="genome", ref_chunk_bytes=4096)
    with pytest.raises(ValueError, match="whole contigs"):
        scan_report(*single, alignable_filter="genome", ref_chunk_bytes=4096)
    with pytest.raises(ValueError, match="one CSV"):                         # multi-CSV mode does not have it
        scan_report("no.fa", "no.txt", "r1.fq", "r2.fq", alignable_filter="genome")
    with pytest.raises(ValueError, match="remove_alignables"):
        scan_report(*pair, alignable_filter="genome", remove_alignables=True)


def test_scan_report_hands_the_switch_to_the_single_csv_scanners(monkeypatch):
    from genefuserust_amd import multi_csv_scan
    seen = []
    monkeypatch.setattr(scan, "scan_pair_end_report", lambda *a, **k: (seen.append(("pair", k)), ([], {}))[1])
    monkeypatch.setattr(scan, "scan_single_end_report", lambda *a, **k: (seen.append(("single", k)), ([], {}))[1])
    multi_csv_scan.scan_report("ref.fa", "x.csv", "r1.fq", "r2.fq", alignable_filter="genome")
    multi_csv_scan.scan_report("ref.fa", "x.csv", "r1.fq", alignable_filter="genome")
    multi_csv_scan.scan_report("ref.fa", "x.csv", "r1.fq", "r2.fq")
    assert [(what, k["alignable_filter"]) for what, k in seen] == [("pair", "genome"), ("single", "genome"), ("pair", None)]


def test_the_command_line_option_reaches_scan_report(monkeypatch, tmp_path, capsys):
    from genefuserust_amd import cli, multi_csv_scan
    a = cli.parser().parse_args(["-1", "a.fq", "-f", "x.csv", "-r", "ref.fa"])
    assert a.alignable_filter is None
    a = cli.parser().parse_args(["-1", "a.fq", "-f", "x.csv", "-r", "ref.fa", "--alignable-filter", "genome"])
    assert a.alignable_filter == "genome"
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["-1", "a.fq", "-f", "x.csv", "-r", "ref.fa", "--alignable-filter", "host"])
    seen = []

    def scan_report(ref, fusion, r1, r2, **kw):
        seen.append(kw)
        return [], {}
    monkeypatch.setattr(multi_csv_scan, "scan_report", scan_report)
    monkeypatch.setattr(multi_csv_scan, "scan_multi_csv_report",
                        lambda *a, **k: (_ for _ in ()).throw(AssertionError("the multi-CSV scan was started")))
    for name in ("ref.fa", "x.csv", "panels.txt", "a.fq", "b.fq"):
        (tmp_path / name).write_text("")
    files = ["-1", str(tmp_path / "a.fq"), "-2", str(tmp_path / "b.fq"), "-r", str(tmp_path / "ref.fa"), "-h", "", "-j", ""]
    assert cli.main(files + ["-f", str(tmp_path / "x.csv"), "--alignable-filter", "genome"]) == 0
    assert cli.main(files + ["-f", str(tmp_path / "x.csv")]) == 0
    assert seen[0]["alignable_filter"] == "genome" and "alignable_filter" not in seen[1]   # off: the call of today
    # multi-CSV mode, streamed, does not have it: refused before the scan starts
    assert cli.main(files + ["-f", str(tmp_path / "panels.txt"), "--chunk-bytes", "4096", "--alignable-filter", "genome"]) == 1
    assert "alignable_filter" in capsys.readouterr().err
