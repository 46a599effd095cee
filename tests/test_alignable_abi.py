"""CPU-side checks of libgfalign.so, the whole-genome alignable filter (include/gf_alignable.h): it loads next to
libgfmatch.so, exports what its header declares with the signatures alignable.py binds, is bound by INTEGRATION.md,
sizes its buffers, rejects bad arguments before it touches a device, and has no CPU fallback.  Plus the host side of
the driver that needs no device: the plan of the pieces and the early returns."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from genefuserust_amd import _lib, alignable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["gf_al_bucket_bytes", "gf_al_filter_bytes", "gf_al_flag_bytes", "gf_al_index_device", "gf_al_last_error",
                "gf_al_scan_device", "gf_al_seeds_device"]


def _header() -> str:
    return open(os.path.join(ROOT, "include", "gf_alignable.h")).read()


def _declarations():
    """{entry point: [parameter type, ...]} of include/gf_alignable.h."""
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(gf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        out[name] = [] if params.strip() == "void" else [" ".join(p.split()[:-1]) for p in params.split(",")]
    return out


def test_header_declares_the_entry_points():
    assert sorted(_declarations()) == ENTRY_POINTS


def test_library_exports_and_signatures_match_the_header():
    L = alignable.lib()
    ctype_of = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    for name, params in _declarations().items():
        assert hasattr(L, name), "libgfalign.so does not export %s" % name
        assert getattr(L, name).argtypes == [C.c_void_p if "*" in p else ctype_of[p] for p in params], name
    assert L.gf_al_last_error.restype == C.c_char_p
    nm = subprocess.run(["nm", "-D", "--defined-only", alignable.AL_LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:   # nothing but the header's functions carries the library's prefix
        exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
        assert {s for s in exported if s.startswith("gf_al_")} == set(ENTRY_POINTS)


def test_library_needs_libgfmatch_next_to_it():
    out = subprocess.run(["readelf", "-d", alignable.AL_LIB_PATH], capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("readelf not available")
    assert "[libgfmatch.so]" in out.stdout and "$ORIGIN" in out.stdout


def test_integration_doc_binds_every_entry_point():
    """INTEGRATION.md's last `extern "C"` block (after the one of gf_report.h) binds every function of gf_alignable.h,
    and its constants are the header's."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = doc.index('extern "C" {', doc.index("pub fn gf_rp_last_error()"))
    assert doc.rindex('extern "C" {') == start
    block = doc[start:doc.index("}", start)]
    assert sorted(set(re.findall(r"pub fn (gf_[a-z0-9_]+)\(", block))) == ENTRY_POINTS
    for name, params in _declarations().items():   # and with as many parameters
        bound = re.search(r"pub fn %s\(([^)]*)\)" % name, block).group(1)
        assert len([p for p in bound.split(",") if p.strip()]) == len(params), name
    defines = dict(re.findall(r"#define (GF_AL_[A-Z0-9_]+) (\d+)", _header()))
    consts = dict(re.findall(r"pub const (GF_AL_[A-Z0-9_]+): \w+ = (\d+);", doc))
    assert consts == defines and len(defines) == 6


def test_constants_are_the_specifications_and_the_drivers():
    defines = {k: int(v) for k, v in re.findall(r"#define (GF_AL_[A-Z0-9_]+) (\d+)", _header())}
    assert defines["GF_AL_WINDOW"] == alignable.K == 16 and defines["GF_AL_UNCOVERED_LIMIT"] == alignable.LIMIT == 10
    assert defines["GF_AL_READS_MAX"] == alignable.READS_MAX
    assert (defines["GF_AL_FILTER_LOG2_MIN"], defines["GF_AL_FILTER_LOG2_MAX"]) == \
        (alignable.FILTER_LOG2_MIN, alignable.FILTER_LOG2_MAX)
    assert defines["GF_AL_SEPARATOR_BYTE"] == alignable.SEPARATOR
    assert alignable.FILTER_LOG2_MIN <= alignable.FILTER_LOG2_DEFAULT <= alignable.FILTER_LOG2_MAX


def test_buffer_sizes():
    L = alignable.lib()
    assert [L.gf_al_filter_bytes(b) for b in (15, 16, 20, 32, 33, -1)] == [0, 1 << 13, 1 << 17, 1 << 29, 0, 0]
    assert L.gf_al_bucket_bytes() % 4 == 0 and L.gf_al_bucket_bytes() >= 4 * 2
    assert [L.gf_al_flag_bytes(n) for n in (-1, 0, 1, 32, 33, 64, 65)] == [0, 0, 4, 4, 8, 8, 12]


def _host_pointer():
    buf = (C.c_char * 512)()
    base = C.addressof(buf)
    return buf, C.c_void_p(base + -base % 16)


def test_argument_errors_without_a_device():
    L = alignable.lib()
    buf, p = _host_pointer()
    ARG, CAP, NODEV = _lib.GF_ERR_ARG, _lib.GF_ERR_CAPACITY, _lib.GF_ERR_NO_DEVICE
    # the seeds
    assert L.gf_al_seeds_device(p, -1, p, 1, p, p, p, 20, None) == ARG and b"negative" in L.gf_al_last_error()
    assert L.gf_al_seeds_device(p, 10, p, -1, p, p, p, 20, None) == ARG
    assert L.gf_al_seeds_device(p, 10, p, alignable.READS_MAX + 1, p, p, p, 20, None) == CAP
    assert b"GF_AL_READS_MAX" in L.gf_al_last_error()
    for bits in (15, 33, 0, -1):
        assert L.gf_al_seeds_device(p, 10, p, 1, p, p, p, bits, None) == ARG and b"filter_log2_bits" in L.gf_al_last_error()
    assert L.gf_al_seeds_device(p, 10, None, 1, p, p, p, 20, None) == ARG and b"offsets" in L.gf_al_last_error()
    assert L.gf_al_seeds_device(p, 10, p, 1, p, p, None, 20, None) == ARG and b"filter" in L.gf_al_last_error()
    for hole in range(3):
        args = [p, 10, p, 1, p, p, p, 20, None]
        args[(0, 4, 5)[hole]] = None
        assert L.gf_al_seeds_device(*args) == ARG and b"null bases, strands or seeds" in L.gf_al_last_error()
    assert L.gf_al_seeds_device(p, 10, p, 1, p, p, p, 20, None) == NODEV       # host memory: there is no CPU fallback
    assert b"no CPU fallback" in L.gf_al_last_error()
    # the entry table
    assert L.gf_al_index_device(p, -1, p, None) == ARG
    assert L.gf_al_index_device(p, 10, None, None) == ARG and b"bucket" in L.gf_al_last_error()
    assert L.gf_al_index_device(None, 10, p, None) == ARG and b"seeds" in L.gf_al_last_error()
    assert L.gf_al_index_device(p, 1 << 40, p, None) == CAP
    assert L.gf_al_index_device(p, 10, p, None) == NODEV

    def scan(text=p, text_bytes=100, strands=p, bases_bytes=50, offsets=p, n=1, seeds=p, buckets=p, filt=p, bits=20, flags=p):
        return L.gf_al_scan_device(text, text_bytes, strands, bases_bytes, offsets, n, seeds, buckets, filt, bits, flags, None)
    assert scan(text_bytes=-1) == ARG and scan(bases_bytes=-1) == ARG and scan(n=-1) == ARG
    assert scan(n=alignable.READS_MAX + 1) == CAP and scan(bits=40) == ARG and scan(offsets=None) == ARG
    assert scan(text=None) == ARG and b"null text" in L.gf_al_last_error()
    assert scan(text=C.c_void_p(p.value + 8)) == ARG and b"aligned" in L.gf_al_last_error()
    for hole in ("strands", "seeds", "buckets", "filt", "flags"):
        assert scan(**{hole: None}) == ARG, hole
    # nothing can be alignable: no text of a window's length, no reads, no bases — nothing is touched
    assert scan(text=None, text_bytes=15) == _lib.GF_OK and scan(n=0, offsets=None) == _lib.GF_OK
    assert scan(bases_bytes=0) == _lib.GF_OK
    assert scan() == NODEV and b"not device memory" in L.gf_al_last_error()
    del buf


def test_the_plan_of_the_pieces():
    plan = alignable.plan_pieces
    assert plan([], 100, 9) == [] and plan([0, 0], 100, 9) == []
    assert plan([30, 40, 28], 100, 9) == [[(0, 0, 30), (1, 0, 40), (2, 0, 28)]]          # 98 bases + 2 separators
    assert plan([30, 40, 29], 100, 9) == [[(0, 0, 30), (1, 0, 40)], [(2, 0, 29)]]         # one byte too many
    assert plan([100], 100, 9) == [[(0, 0, 100)]]
    assert plan([101], 100, 9) == [[(0, 0, 100)], [(0, 91, 101)]]
    assert plan([10, 250, 5], 100, 9) == [[(0, 0, 10)], [(1, 0, 100)], [(1, 91, 191)], [(1, 182, 250), (2, 0, 5)]]
    # every stretch of overlap + 1 bases of a contig lies whole in one piece; no piece is larger than asked
    rng = np.random.default_rng(6)
    for _ in range(50):
        lengths = rng.integers(0, 700, int(rng.integers(1, 8))).tolist()
        piece, overlap = int(rng.integers(40, 300)), int(rng.integers(0, 39))
        pieces = plan(lengths, piece, overlap)
        assert all(sum(e - s for _, s, e in parts) + len(parts) - 1 <= piece for parts in pieces)
        for k, n in enumerate(lengths):
            spans = [(s, e) for parts in pieces for c, s, e in parts if c == k]
            assert (not spans) == (n == 0)
            for a in range(0, n - overlap):
                assert any(s <= a and a + overlap + 1 <= e for s, e in spans), (lengths, piece, overlap, k, a)
            if 0 < n <= overlap:
                assert spans == [(0, n)]


def test_nothing_to_do_needs_no_device(monkeypatch):
    """No reads, no reference, only reads shorter than a window: all False, and neither torch nor the library is
    asked for anything."""
    def boom(*a, **k):
        raise AssertionError("the device was asked")
    monkeypatch.setattr(alignable, "lib", boom)
    monkeypatch.setattr(alignable, "_torch_device", boom)
    ref = {"chr": b"ACGT" * 100}
    assert alignable.alignable_reads_device(ref, []).tolist() == []
    assert alignable.alignable_reads_device(None, [b"ACGT" * 10]).tolist() == [False]
    assert alignable.alignable_reads_device({}, [b"ACGT" * 10, b""]).tolist() == [False, False]
    assert alignable.alignable_reads_device(ref, [b"ACGTACGTACGTACG", b""]).tolist() == [False, False]
    stats = {}
    alignable.alignable_reads_device(ref, [], stats=stats)
    assert stats == {"scan_ms": [], "text_bytes": 0, "pieces": 0, "seeds": 0}
    with pytest.raises(ValueError, match="filter_log2_bits"):
        alignable.alignable_reads_device(ref, [b"A" * 20], filter_log2_bits=12)
    with pytest.raises(ValueError, match="batch_bytes"):
        alignable.alignable_reads_device(ref, [b"A" * 20], batch_bytes=0)
    with pytest.raises(_lib.GfError) as e:
        alignable.alignable_reads_device(ref, [b"A" * 4097])
    assert e.value.code == _lib.GF_ERR_READ_TOO_LONG


def test_no_cpu_fallback(monkeypatch):
    """Without a GPU the call raises: nothing is computed on the host."""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.GfError) as e:
        alignable.alignable_reads_device({"chr": b"ACGT" * 100}, [b"ACGT" * 10])
    assert e.value.code == _lib.GF_ERR_NO_DEVICE
