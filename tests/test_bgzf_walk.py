"""gf_if_walk_blocks (include/gf_inflate.h), the host half of libgfinflate.so, without a GPU: held to
``tests/bgzf_members.walk_model`` on member series of every shape; and the library's exports, header and DT_NEEDED."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from tests import bgzf_members as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["gf_if_copy_from_host_device", "gf_if_inflate_device", "gf_if_last_error", "gf_if_walk_blocks",
                "gf_if_workspace_bytes"]

A, B, C3 = bm.fastq_text(3000, 1), bm.fastq_text(70, 2), b"x"
FOREIGN = b"XY\x03\x00abc"      # an extra subfield of another kind, three bytes long


def series():
    m = bm.member
    return {
        "plain": [m(A), m(B), m(C3), bm.EOF_MARKER],
        "no_marker": [m(A), m(B)],
        "marker_in_the_middle": [m(A), bm.EOF_MARKER, m(b""), m(B), bm.EOF_MARKER, bm.EOF_MARKER],
        "only_markers": [bm.EOF_MARKER, bm.EOF_MARKER],
        "foreign_subfield": [m(A, extra_front=FOREIGN), m(B, extra_front=FOREIGN + FOREIGN), bm.EOF_MARKER],
        "plain_gzip_first": [gzip.compress(A), m(B)],
        "plain_gzip_second": [m(A), gzip.compress(B), m(B)],
        "empty": [],
    }


def same(comp: bytes, **kw):
    from genefuserust_amd import bgzf
    rows, comp_bytes, text, why, stop = bm.walk_model(comp, **kw)
    w = bgzf.walk_blocks(comp, **kw)
    assert (w.table.tolist(), w.comp_bytes, w.text_bytes, w.why, w.stop) == (rows, comp_bytes, text, why, stop), kw
    return w


@pytest.mark.parametrize("name", sorted(series()))
def test_walk_is_the_model(name):
    members = series()[name]
    comp = b"".join(members)
    w = same(comp)
    same(comp, file_offset=12345)
    if "plain_gzip" not in name:
        assert w.why == bm.WALK_END and w.members == len(members) and w.comp_bytes == len(comp)
        # the rows are the members: payloads inflate to the texts zlib gives
        text = gzip.decompress(comp) if comp else b""
        for row in w.table:
            import zlib
            got = zlib.decompress(comp[row[0]:row[0] + row[1]], -15)
            assert got == text[row[2]:row[2] + row[3]] and zlib.crc32(got) == row[4]
    else:
        first = name.endswith("first")
        assert w.why == bm.WALK_NOT_BGZF and w.members == (0 if first else 1) and w.stop == (0 if first else len(members[0]))
    for cap in range(len(members) + 1):
        c = same(comp, max_members=cap)
        assert c.members <= cap


def test_text_budget_at_and_around_a_member():
    members = series()["marker_in_the_middle"]
    comp = b"".join(members)
    for budget, n in ((len(A), 3), (len(A) - 1, 0), (len(A) + 1, 3), (len(A) + len(B), 6), (len(A) + len(B) - 1, 3), (0, 0)):
        w = same(comp, text_budget=budget)
        assert w.members == n, budget
        assert w.why == (bm.WALK_END if n == 6 else bm.WALK_BUDGET)
    # empty members fit any budget
    assert same(b"".join(series()["only_markers"]), text_budget=0).members == 2


def test_a_range_cut_anywhere():
    """Every cut of a three-member series: inside a header, the extra field, a payload, a trailer."""
    members = [bm.member(B, extra_front=FOREIGN), bm.member(C3), bm.EOF_MARKER]
    comp = b"".join(members)
    ends = np.cumsum([len(m) for m in members]).tolist()
    for cut in range(len(comp) + 1):
        w = same(comp[:cut])
        whole = sum(1 for e in ends if e <= cut)
        assert w.members == whole and w.why == (bm.WALK_END if cut in [0] + ends else bm.WALK_INSIDE), cut
    # bytes that cannot begin a member are told apart as soon as they are seen
    for junk in (b"\x1f\x8c", b"\x1f\x8b\x08\x00" + b"\0" * 30, b"@read\n"):
        w = same(members[0] + junk)
        assert w.why == bm.WALK_NOT_BGZF and w.stop == len(members[0])
    # a BC subfield of another length, a block size that cannot hold the framing, an ISIZE beyond 64 KiB
    odd = bytearray(members[1])
    odd[14] = 3
    assert same(bytes(odd)).why == bm.WALK_NOT_BGZF
    short = bytearray(members[1])
    short[16:18] = (20).to_bytes(2, "little")
    assert same(bytes(short)).why == bm.WALK_NOT_BGZF
    big = bytearray(members[1])
    big[-4:] = (65537).to_bytes(4, "little")
    assert same(bytes(big)).why == bm.WALK_NOT_BGZF


def test_argument_errors():
    from genefuserust_amd import _lib, bgzf
    L = bgzf.lib()
    res = (C.c_int64 * 5)()
    table = (C.c_int64 * 6)()
    buf = C.create_string_buffer(bm.EOF_MARKER, 28)
    assert L.gf_if_walk_blocks(buf, 28, 0, 0, 1, table, None) == _lib.GF_ERR_ARG
    assert L.gf_if_walk_blocks(None, 28, 0, 0, 1, table, res) == _lib.GF_ERR_ARG
    assert L.gf_if_walk_blocks(buf, 28, 0, 0, 1, None, res) == _lib.GF_ERR_ARG
    assert b"null" in L.gf_if_last_error()
    for args in ((-1, 0, 0, 1), (28, -1, 0, 1), (28, 0, -1, 1), (28, 0, 0, -1)):
        assert L.gf_if_walk_blocks(buf, args[0], args[1], args[2], args[3], table, res) == _lib.GF_ERR_ARG
        assert b"negative" in L.gf_if_last_error()
    assert L.gf_if_walk_blocks(buf, 28, 7, 0, 1, table, res) == 0
    assert list(res) == [1, 28, 0, bm.WALK_END, 28] and list(table) == [18, 2, 0, 0, 0, 7]
    # the device call refuses host memory and bad sizes before it touches a device
    assert L.gf_if_workspace_bytes(1000) >= 0
    tot = (C.c_int64 * 4)()
    st = (C.c_int32 * 1)()
    assert L.gf_if_inflate_device(buf, 28, table, 1, buf, 0, st, tot, None, 0, None) == _lib.GF_ERR_NO_DEVICE
    assert b"not device memory" in L.gf_if_last_error()
    assert L.gf_if_inflate_device(buf, -1, table, 1, buf, 0, st, tot, None, 0, None) == _lib.GF_ERR_ARG
    assert L.gf_if_inflate_device(buf, 28, None, 1, buf, 0, st, tot, None, 0, None) == _lib.GF_ERR_ARG
    assert L.gf_if_inflate_device(buf, 28, table, 1, buf, 0, st, None, None, 0, None) == _lib.GF_ERR_ARG
    assert L.gf_if_copy_from_host_device(buf, buf, 28, None) == _lib.GF_ERR_NO_DEVICE
    assert L.gf_if_copy_from_host_device(buf, buf, -1, None) == _lib.GF_ERR_ARG


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "gf_inflate.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gf_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_entry_points():
    assert _declared_functions() == ENTRY_POINTS


def test_library_exports_every_declared_symbol():
    from genefuserust_amd import bgzf
    L = bgzf.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), "libgfinflate.so does not export %s" % name


def test_library_needs_libgfmatch_next_to_it():
    out = subprocess.run(["readelf", "-d", os.path.join(ROOT, "genefuserust_amd", "libgfinflate.so")],
                         capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("readelf not available")
    assert "[libgfmatch.so]" in out.stdout and "$ORIGIN" in out.stdout


def test_integration_doc_binds_every_entry_point():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = doc.index('extern "C" {', doc.index("gf_inflate.h"))
    block = doc[start:doc.index("}", start)]
    assert sorted(set(re.findall(r"pub fn (gf_[a-z0-9_]+)\(", block))) == ENTRY_POINTS


def test_statuses_are_the_cores():
    """tests/bgzf_members.py, bgzf.STATUS_TEXT and gf_if_core.h name the same statuses."""
    from genefuserust_amd import bgzf
    core = open(os.path.join(ROOT, "genefuserust_amd", "scan_csrc", "gf_if_core.h")).read()
    found = dict((name, int(v)) for name, v in re.findall(r"^#define GF_IF_([A-Z_]+) (\d+)\b", core, flags=re.M))
    for name in ("OK", "BAD_BTYPE", "STORED_LEN", "BAD_COUNTS", "OVERSUBSCRIBED", "INCOMPLETE", "REPEAT_FIRST",
                 "LENGTHS_OVERRUN", "NO_END_CODE", "BAD_LITLEN", "BAD_DIST_SYM", "DIST_TOO_FAR", "OUTPUT_OVERRUN",
                 "OUTPUT_SHORT", "INPUT_EXHAUSTED", "CRC", "BAD_ROW", "BAD_CODE", "TRAILING"):
        assert found[name] == getattr(bm, name), name
    assert sorted(bgzf.STATUS_TEXT) == list(range(1, 19))
    assert found["ROW"] == bm.ROW == bgzf.ROW and found["MAX_TEXT"] == bm.MAX_TEXT == bgzf.MAX_TEXT
