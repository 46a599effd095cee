"""The shared pieces of the file-level scans (scan.py, read_pair.scan_with_room) without a GPU and without any of the
libraries: the overflow retry over stub scans, the naming rule, and the counters of every route — keys and their order
— through the match tail with a stub mapper."""
import pytest


class _Res:
    """What a scan returns as far as ``scan_with_room`` looks: ``download()``."""

    def __init__(self, caps, overflow, log):
        self.caps, self.overflow, self.log = caps, overflow, log

    def download(self):
        self.log.append(("download", self.caps))
        return ("rec", b"bases", b"quals", {"overflow": self.overflow, "hits": len(self.log)})


def _stub_scan(overflows, log):
    it = iter(overflows)

    def scan(**caps):
        log.append(("scan", caps))
        return _Res(caps, next(it), log)
    return scan


FIRST = dict(hits_cap=1024, bytes_cap=4096)
ROOM = dict(hits_cap=30, bytes_cap=2064, retry_cap=30)


def test_retry_scans_once_when_nothing_overflows():
    from genefuserust_amd.read_pair import scan_with_room
    log = []
    res, behind, out = scan_with_room(_stub_scan([0], log), FIRST, ROOM)
    assert log == [("scan", FIRST), ("download", FIRST)]
    assert res.caps == FIRST and behind is None and out[3]["overflow"] == 0 and out[:3] == ("rec", b"bases", b"quals")


@pytest.mark.parametrize("bits", [1, 2, 3])
def test_retry_scans_again_with_exactly_the_room_capacities(bits):
    from genefuserust_amd.read_pair import scan_with_room
    log = []
    res, behind, out = scan_with_room(_stub_scan([bits, 0], log), FIRST, ROOM)
    assert log == [("scan", FIRST), ("download", FIRST), ("scan", ROOM), ("download", ROOM)]
    assert res.caps == ROOM and out[3] == {"overflow": 0, "hits": 4}
    # the first attempt of the streamed route: the library's defaults, no capacity at all
    log = []
    scan_with_room(_stub_scan([bits, 0], log), {}, ROOM)
    assert [x for x in log if x[0] == "scan"] == [("scan", {}), ("scan", ROOM)]


def test_retry_raises_when_the_second_scan_overflows_too():
    from genefuserust_amd import _lib
    from genefuserust_amd.read_pair import scan_with_room
    log = []
    with pytest.raises(_lib.GfError) as e:
        scan_with_room(_stub_scan([2, 2, 0], log), FIRST, ROOM)
    assert e.value.code == _lib.GF_ERR_CAPACITY
    assert [x[0] for x in log] == ["scan", "download", "scan", "download"]   # and no third attempt


@pytest.mark.parametrize("overflows", [[0], [1, 0]])
def test_retry_queues_work_between_each_scan_and_its_download(overflows):
    from genefuserust_amd.read_pair import scan_with_room
    log = []

    def behind(res):
        log.append(("behind", res.caps))
        return "names of %d" % len(res.caps)
    res, got, out = scan_with_room(_stub_scan(overflows, log), FIRST, ROOM, behind)
    caps = [FIRST, ROOM][:len(overflows)]
    assert log == [(what, c) for c in caps for what in ("scan", "behind", "download")]
    assert got == "names of %d" % len(caps[-1]) and res.caps == caps[-1]   # what was queued behind the scan that counts


class _Match:
    def __init__(self, source, merge_diff=-1):
        self.m_source, self.m_merge_diff, self.m_name = source, merge_diff, b""


def test_the_naming_rule():
    from genefuserust_amd.scan import match_named
    asked = []

    def name_of_side(side):
        asked.append(side)
        return {"r1": b"@read/1", "r2": b"@read/2"}[side]
    m = _Match("r1")
    assert match_named(m, name_of_side) is m and m.m_name == b"@read/1"
    assert match_named(_Match("r2"), name_of_side).m_name == b"@read/2"
    assert match_named(_Match("merged", 0), name_of_side).m_name == b"@read/1 merged_diff_0"
    assert match_named(_Match("merged", -37), name_of_side).m_name == b"@read/1 merged_diff_-37"
    assert asked == ["r1", "r2", "r1", "r1"]   # one name is cut per match, the one it carries


def test_names_from_the_host_texts_and_from_the_device(monkeypatch):
    from genefuserust_amd import scan
    monkeypatch.setattr(scan, "record_lines", lambda batch, text, i: (b"@%s:%s:%d" % (batch, text, i), b"", b"", b""))
    hits = [(0, _Match("r1")), (0, _Match("r2")), (4, _Match("merged", 3)), (7, _Match("r2"))]
    found = scan.named_from_records(hits, b"L", b"lt", b"R", b"rt")
    assert found == [m for _, m in hits]
    assert [m.m_name for m in found] == [b"@L:lt:0", b"@R:rt:0", b"@L:lt:4 merged_diff_3", b"@R:rt:7"]
    assert scan.named_from_records([(2, _Match("r1"))], b"L", b"lt")[0].m_name == b"@L:lt:2"   # single-end: no R2
    # streamed: one gathered name per record (source 0 merged, 1 r1, 2 r2), pair ids counted from the start of the file
    hits = [(100, _Match("r1")), (100, _Match("r2")), (104, _Match("merged", 3)), (107, _Match("r2"))]
    rec = [{"pair_id": 100, "source": 1}, {"pair_id": 100, "source": 2}, {"pair_id": 104, "source": 0},
           {"pair_id": 105, "source": 1},   # (a record whose tail gave no match)
           {"pair_id": 107, "source": 2}]
    names = [b"@p100/1", b"@p100/2", b"@p104/1", b"@p105/1", b"@p107/2"]
    assert [m.m_name for m in scan.named_from_device(hits, rec, names)] == \
        [b"@p100/1", b"@p100/2", b"@p104/1 merged_diff_3", b"@p107/2"]


class _Mapper:
    """``filter_matches`` drops the matches named b"drop"; ``sort_matches`` reverses; both note that they ran."""

    def __init__(self):
        self.calls = []

    def filter_matches(self, found, deletion_threshold):
        self.calls.append(("filter", deletion_threshold))
        kept = [m for m in found if m != b"drop"]
        return kept, {"complexity": len(found) - len(kept), "distance": 0, "indels": 0}

    def remove_alignables(self, kept):
        self.calls.append(("alignables",))
        return kept[1:], 1

    def sort_matches(self, kept):
        self.calls.append(("sort",))
        return kept[::-1]


FILTER_KEYS = ["complexity", "distance", "indels"]
TOT = {"hits": 9, "hit_bytes": 900, "merged_pairs": 5, "retried_reads": 2, "overflow": 0}
ROUTES = [   # (arguments of route_counters after n_found, keys in front of the filter counts, keys behind them)
    ("pairs, whole file", ("pairs", TOT, None), ["pairs", "matches_before_filtering", "merged_pairs", "retried_reads"], []),
    ("pairs, streamed", ("pairs", TOT, 3), ["pairs", "matches_before_filtering", "merged_pairs", "retried_reads"],
     ["chunks"]),
    ("single-end, device", ("reads", TOT, None), ["reads", "matches_before_filtering"], ["retried_reads"]),
    ("single-end, host", ("reads", None, None), ["reads", "matches_before_filtering"], []),
    ("single-end, streamed", ("reads", TOT, 3), ["reads", "matches_before_filtering"], ["retried_reads", "chunks"]),
]


@pytest.mark.parametrize("alignables", [False, True])
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_counters_of_every_route_keys_and_order(route, alignables):
    from genefuserust_amd.scan import finish_matches, report_matches, route_counters
    _, (count_key, tot, chunks), front, back = route
    found = [b"a", b"drop", b"b", b"c"]
    before, after = route_counters(count_key, 150, len(found), tot, chunks)
    mapper = _Mapper()
    kept, counters = finish_matches(found, mapper, 50, alignables, before, after)
    assert list(counters) == front + FILTER_KEYS + (["alignables"] if alignables else []) + back
    assert mapper.calls == [("filter", 50)] + ([("alignables",)] if alignables else []) + [("sort",)]
    assert kept == ([b"c", b"b"] if alignables else [b"c", b"b", b"a"])
    want = {count_key: 150, "matches_before_filtering": 4, "complexity": 1, "distance": 0, "indels": 0}
    if count_key == "pairs":
        want["merged_pairs"] = 5
    if tot is not None:
        want["retried_reads"] = 2
    if chunks is not None:
        want["chunks"] = 3
    if alignables:
        want["alignables"] = 1
    assert counters == want
    # the report tail appends ``fusions`` (no match, no fusion: the clustering needs no library for an empty list)
    from genefuserust_amd import Settings
    order = list(counters)
    results, with_fusions = report_matches([], counters, [], [], Settings())
    assert results == [] and list(with_fusions) == order + ["fusions"] and with_fusions["fusions"] == 0
