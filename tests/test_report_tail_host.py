"""The host half of the bulk report tail (genefuserust_amd/report_tail.py, include/gf_report.h) without a GPU:
``first_fit`` against the literal first-fit loop of ``cluster_matches``, ``order_matches`` against ``sort_matches``, and
libgfreport.so's header, exports and ctypes signatures against one another."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from genefuserust_amd import GenePos, ReadMatch, _lib, report_tail
from genefuserust_amd.fusion_mapper import FusionMapper
from genefuserust_amd.fusion_result import first_fit_clusters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def match(lp, rp, brk=30, read=b"A" * 60, name=b"@r"):
    return ReadMatch(read, brk, GenePos(0, int(lp)), GenePos(1, int(rp)), 1, 0, 0, m_name=name)


def literal_founders(groups):
    """Per match (all groups, flattened) the index of its cluster's first match, by the literal loop."""
    flat = [m for g in groups for m in g]
    index = {id(m): k for k, m in enumerate(flat)}
    out = [None] * len(flat)
    for fr in first_fit_clusters(groups):
        for m in fr.m_matches:
            out[index[id(m)]] = index[id(fr.m_matches[0])]
    return out


def bulk_founders(groups):
    flat = [m for g in groups for m in g]
    off = np.cumsum([0] + [len(g) for g in groups])
    return report_tail.first_fit([m.m_left_gp.position for m in flat], [m.m_right_gp.position for m in flat], off).tolist()


def test_first_fit_takes_the_first_cluster_not_the_nearest_match():
    # A(0) founds, B(6) founds, C(3) is within 3 of both: it joins A's cluster
    g = [match(0, 100), match(6, 100), match(3, 100)]
    assert bulk_founders([g]) == literal_founders([g]) == [0, 1, 0]
    # and through C a later D(6) reaches A's cluster although B sits in D's own cell
    g.append(match(6, 100))
    assert bulk_founders([g]) == literal_founders([g]) == [0, 1, 0, 0]


def test_first_fit_keeps_a_cells_smallest_founder():
    """A cell written by matches of different founders answers with the smallest.  (A later match in a cell sees that
    cell, so its founder is never larger than the cell's: the founders written to one cell only go down, and the
    smallest is the last one written.  What can go wrong is keeping the first.)"""
    # X founds cluster 1 in cell (6, 0); B bridges A's cluster to that cell; Y, in X's cell, joins A's cluster;
    # Z sees nothing but cell (6, 0) and must find A's cluster there, not X's
    g = [match(0, 0), match(6, 0), match(3, 0), match(6, 0), match(9, 0)]
    assert literal_founders([g]) == [0, 1, 0, 0, 0] and bulk_founders([g]) == [0, 1, 0, 0, 0]
    # the same on the right position, with a bystander cluster in between
    g = [match(0, 0), match(0, 6), match(50, 50), match(0, 3), match(0, 6), match(50, 53), match(0, 9), match(3, 9)]
    assert bulk_founders([g]) == literal_founders([g]) == [0, 1, 2, 0, 0, 2, 0, 0]


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_first_fit_on_colliding_random_groups(seed):
    rng = np.random.default_rng(seed)
    sizes = [900, 0, 1200, 1, 899]
    groups = [[match(rng.integers(-20, 20), rng.integers(1000, 1040)) for _ in range(n)] for n in sizes]
    want = literal_founders(groups)
    assert bulk_founders(groups) == want
    assert 5 < len(set(want)) < 600     # clusters collide and merge: far fewer than matches


def test_first_fit_edges():
    assert report_tail.first_fit([], [], [0]).size == 0                 # n = 0
    assert report_tail.first_fit([], [], [0, 0, 0]).size == 0           # empty groups
    assert report_tail.first_fit(np.zeros(0), np.zeros(0), np.zeros(1)).dtype == np.int64
    lo, hi = -2**31, 2**31 - 1                                           # the cells next to them do not wrap
    g = [match(lo, hi), match(lo + 3, hi - 3), match(hi, lo), match(lo + 4, hi), match(-1, 1), match(1, -1), match(2, 2)]
    assert bulk_founders([g]) == literal_founders([g]) == [0, 0, 2, 0, 4, 4, 4]
    # the same positions in two groups never meet
    assert bulk_founders([[match(5, 5)], [match(5, 5), match(6, 6)]]) == [0, 1, 1]
    L = report_tail.lib()
    assert L.gf_rp_first_fit(None, None, None, 1, None) == _lib.GF_ERR_ARG and b"null" in L.gf_rp_last_error()
    assert L.gf_rp_first_fit(None, None, None, -1, None) == _lib.GF_ERR_ARG
    off = np.array([0, 2, 1], dtype=np.int64)
    assert L.gf_rp_first_fit(None, None, off.ctypes.data, 2, None) == _lib.GF_ERR_ARG
    assert b"decrease" in L.gf_rp_last_error()


def test_order_matches_is_sort_matches():
    rng = np.random.default_rng(9)
    names = [b"@run7:lane%d:%d" % (k % 3, k % 11) for k in range(40)] + [b"@run7", b"@run7:", b"", b"@run7:lane1:3/1"]
    ms = [ReadMatch(b"A" * int(rng.integers(58, 62)), int(rng.integers(28, 32)), GenePos(0, k), GenePos(1, k), 0, 0, 0,
                    m_name=names[int(rng.integers(0, len(names)))]) for k in range(2000)]
    want = FusionMapper.sort_matches(ms)
    got = report_tail.order_matches(ms)
    assert [id(m) for m in got] == [id(m) for m in want]      # the same objects: equal keys keep their order
    keys = [(m.m_read_break, len(m.m_read)) for m in ms]
    assert len(set(keys)) <= 16 and len({(k, m.m_name) for k, m in zip(keys, ms)}) < 1000   # many ties, equal names
    assert report_tail.order_matches([]) == [] and report_tail.order_matches(ms[:1]) == ms[:1]


def test_match_table():
    ms = [match(5, -7, 3, b"ACGTA"), match(-2, 9, 0, b""), match(1, 2, 6, b"GGGTTTCCC")]
    ms[2].m_left_distance, ms[2].m_right_distance, ms[2].m_gap = 2, 3, 4
    t = report_tail.MatchTable.from_matches(ms)
    assert len(t) == 3 and t.bases.tobytes() == b"ACGTAGGGTTTCCC" and t.offsets.tolist() == [0, 5, 5, 14]
    assert t.lengths.tolist() == [5, 0, 9] and t.rm.dtype == _lib.READMATCH_DTYPE
    assert t.rm[2].tolist() == (6, 4, 2, 3, 1, 2, 0, 1) and t.rm["left_position"].tolist() == [5, -2, 1]
    empty = report_tail.MatchTable.from_matches([])
    assert len(empty) == 0 and empty.offsets.tolist() == [0] and empty.bases.size == 0


# ---- header <-> exports <-> ctypes ------------------------------------------------------------------------------------

def _declarations():
    """{entry point: [parameter type, ...]} of include/gf_report.h."""
    src = open(os.path.join(ROOT, "include", "gf_report.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(gf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        out[name] = [] if params.strip() == "void" else [" ".join(p.split()[:-1]) for p in params.split(",")]
    return out


def test_header_declares_the_entry_points():
    assert sorted(_declarations()) == ["gf_rp_adjust_device", "gf_rp_filter_device", "gf_rp_first_fit",
                                       "gf_rp_last_error"]


def test_library_exports_and_signatures_match_the_header():
    L = report_tail.lib()
    ctype_of = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    for name, params in _declarations().items():
        assert hasattr(L, name), "libgfreport.so does not export %s" % name
        want = [C.c_void_p if "*" in p else ctype_of[p] for p in params]
        assert getattr(L, name).argtypes == want, name
    assert L.gf_rp_last_error.restype == C.c_char_p
    nm = subprocess.run(["nm", "-D", "--defined-only", report_tail.RP_LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:   # nothing but the header's functions carries the library's prefix
        exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
        assert {s for s in exported if s.startswith("gf_rp_")} == set(_declarations())


def test_library_needs_libgfmatch_next_to_it():
    out = subprocess.run(["readelf", "-d", report_tail.RP_LIB_PATH], capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("readelf not available")
    assert "[libgfmatch.so]" in out.stdout and "$ORIGIN" in out.stdout


def test_argument_errors_and_no_cpu_fallback():
    L = report_tail.lib()
    buf = (C.c_char * 256)()
    p = C.cast(buf, C.c_void_p)
    assert L.gf_rp_filter_device(p, -1, p, p, 1, 50, p, None) == _lib.GF_ERR_ARG and b"negative" in L.gf_rp_last_error()
    assert L.gf_rp_filter_device(p, 10, None, p, 1, 50, p, None) == _lib.GF_ERR_ARG
    assert L.gf_rp_filter_device(None, 10, p, p, 1, 50, p, None) == _lib.GF_ERR_ARG and b"bases" in L.gf_rp_last_error()
    assert L.gf_rp_filter_device(None, 0, None, None, 0, 50, None, None) == _lib.GF_OK          # nothing to do
    assert L.gf_rp_adjust_device(p, 10, p, p, p, 1, p, -1, p, 1, p, None) == _lib.GF_ERR_ARG
    assert L.gf_rp_adjust_device(None, 0, None, None, None, 0, None, 0, None, 0, None, None) == _lib.GF_OK
    # host memory is refused: there is no CPU fallback
    assert L.gf_rp_filter_device(p, 10, p, p, 1, 50, p, None) == _lib.GF_ERR_NO_DEVICE
    assert L.gf_rp_adjust_device(p, 10, p, p, p, 1, p, 10, p, 1, p, None) == _lib.GF_ERR_NO_DEVICE
    assert b"no CPU fallback" in L.gf_rp_last_error()


def test_tail_switch_is_checked_before_any_file_is_opened():
    from genefuserust_amd.multi_csv_scan import scan_multi_csv_report, scan_report
    from genefuserust_amd.scan import (scan_pair_end_files, scan_pair_end_report, scan_single_end_files,
                                       scan_single_end_report)
    for call in (lambda: scan_pair_end_files("no.fa", "no.csv", "r1.fq", "r2.fq", tail="nope"),
                 lambda: scan_pair_end_report("no.fa", "no.csv", "r1.fq", "r2.fq", tail="nope"),
                 lambda: scan_single_end_files("no.fa", "no.csv", "r1.fq", tail="nope"),
                 lambda: scan_single_end_report("no.fa", "no.csv", "r1.fq", tail="nope"),
                 lambda: scan_multi_csv_report("no.fa", "no.txt", "r1.fq", "r2.fq", tail="nope"),
                 lambda: scan_report("no.fa", "no.csv", "r1.fq", "r2.fq", tail="nope"),
                 lambda: scan_report("no.fa", "no.txt", "r1.fq", tail="nope")):
        with pytest.raises(ValueError, match="tail"):
            call()
