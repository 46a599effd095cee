"""CPU-side checks of libgfqc.so, the read QC (include/gf_read_qc.h): it loads next to libgfmatch.so, exports what its
header declares with the signatures read_qc.py binds, is bound by INTEGRATION.md, its constants are the bindings',
it refuses bad arguments before it touches a device, and has no CPU fallback."""
import ctypes as C
import os
import re
import subprocess

import pytest

from genefuserust_amd import _lib, read_qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["gf_qc_insert_device", "gf_qc_last_error", "gf_qc_stats_device"]


def _header() -> str:
    return open(os.path.join(ROOT, "include", "gf_read_qc.h")).read()


def _declarations():
    """{entry point: [parameter type, ...]} of include/gf_read_qc.h."""
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(gf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        out[name] = [] if params.strip() == "void" else [" ".join(p.split()[:-1]) for p in params.split(",")]
    return out


def _defines() -> dict:
    return {k: int(v) for k, v in re.findall(r"#define (GF_QC_[A-Z0-9_]+) (\d+)", _header())}


def test_header_declares_the_entry_points():
    d = _declarations()
    assert sorted(d) == ENTRY_POINTS
    assert len(d["gf_qc_stats_device"]) == 7 and len(d["gf_qc_insert_device"]) == 8
    # the definitions are stated, the way gf_read_filter.h states its predicate
    for phrase in ("phred(j) = max(q[j] - 33, 0)", "length_hist", "min(L, C)", "qual_sum", "ADD into",
                   "hist[GF_QC_INSERT_UNMEASURED]", "ov(I) >= 30, d(I) <= 5 and 100 d(I) <= 20 ov(I)"):
        assert phrase in _header(), phrase


def test_library_exports_and_signatures_match_the_header():
    L = read_qc.lib()
    ctype_of = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    for name, params in _declarations().items():
        assert hasattr(L, name), "libgfqc.so does not export %s" % name
        assert getattr(L, name).argtypes == [C.c_void_p if "*" in p else ctype_of[p] for p in params], name
    assert L.gf_qc_last_error.restype == C.c_char_p
    assert L.gf_qc_stats_device.restype == C.c_int and L.gf_qc_insert_device.restype == C.c_int
    nm = subprocess.run(["nm", "-D", "--defined-only", read_qc.QC_LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:   # nothing but the header's functions carries the library's prefix
        exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
        assert {s for s in exported if s.startswith("gf_qc_")} == set(ENTRY_POINTS)


def test_library_needs_libgfmatch_next_to_it():
    out = subprocess.run(["readelf", "-d", read_qc.QC_LIB_PATH], capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("readelf not available")
    assert "[libgfmatch.so]" in out.stdout and "$ORIGIN" in out.stdout


def test_makefile_builds_the_library_with_the_others():
    mk = open(os.path.join(ROOT, "genefuserust_amd", "scan_csrc", "Makefile")).read()
    for target in ("all:", "resource-usage:", "\trm -f"):
        line = next(x for x in mk.splitlines() if x.startswith(target))
        assert "gfqc" in line or "gf_read_qc.hip" in line, target
    assert "../libgfqc.so: gf_read_qc.hip $(HDRS) ../libgfmatch.so" in mk
    assert "-c -o /dev/null gf_read_qc.hip" in mk and "libgfqc.so" in mk.split("HIPCC ?=")[0]


def test_integration_doc_binds_every_entry_point():
    """INTEGRATION.md's `extern "C"` block for gf_read_qc.h binds every function of the header, with as many
    parameters, and its constants are the header's."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = doc.index('extern "C" {', doc.index("src/gfqc_sys.rs"))
    block = doc[start:doc.index("}", start)]
    assert sorted(set(re.findall(r"pub fn (gf_[a-z0-9_]+)\(", block))) == ENTRY_POINTS
    for name, params in _declarations().items():
        bound = re.search(r"pub fn %s\(([^)]*)\)" % name, block).group(1)
        assert len([p for p in bound.split(",") if p.strip()]) == len(params), name
    consts = {k: int(v) for k, v in re.findall(r"pub const (GF_QC_[A-Z0-9_]+): \w+ = (\d+);", doc)}
    assert consts == _defines() and len(consts) == 14


def test_constants_are_the_bindings():
    d = _defines()
    assert d["GF_QC_CYCLES"] == read_qc.CYCLES == 512 and d["GF_QC_COLUMNS"] == read_qc.COLUMNS == 8
    assert d["GF_QC_SIDE_WORDS"] == read_qc.SIDE_WORDS == 513 + 513 * 8 == 4617
    assert d["GF_QC_INSERT_WORDS"] == read_qc.INSERT_WORDS == 1026
    assert d["GF_QC_INSERT_UNMEASURED"] == read_qc.INSERT_UNMEASURED == 1025
    assert d["GF_QC_INSERT_MIN"] == read_qc.INSERT_MIN == 30
    cols = ("A", "C", "G", "T", "N", "QUAL_SUM", "Q20", "Q30")
    assert [d["GF_QC_COL_" + c] for c in cols] == [getattr(read_qc, "COL_" + c) for c in cols] == list(range(8))
    # the kernels' constants: what the GPU tests size their batches by
    kernels = open(os.path.join(ROOT, "genefuserust_amd", "scan_csrc", "gf_qc_kernels.h")).read()
    assert re.search(r"#define GF_QC_GRID (\d+)", kernels).group(1) == "768"
    core = open(os.path.join(ROOT, "genefuserust_amd", "scan_csrc", "gf_qc_core.h")).read()
    assert "#define GF_QC_FLUSH_RECORDS (1 << 20)" in core and 222 * (1 << 20) < 1 << 28


def _stats(L, idx=True, n=10, **null):
    """gf_qc_stats_device over host memory that is never dereferenced: the checks come first."""
    buf = (C.c_char * 256)()
    dummy = C.cast(buf, C.c_void_p)
    p = lambda name: None if null.get(name) else dummy   # noqa: E731
    return L.gf_qc_stats_device(dummy if idx else None, p("bases"), p("quals"), p("off"), n, p("table"), None)


def _insert(L, idx=True, n=10, **null):
    buf = (C.c_char * 256)()
    dummy = C.cast(buf, C.c_void_p)
    p = lambda name: None if null.get(name) else dummy   # noqa: E731
    return L.gf_qc_insert_device(dummy if idx else None, p("l_bases"), p("l_off"), p("r_bases"), p("r_off"), n,
                                 p("hist"), None)


def test_argument_errors_without_a_device():
    L = read_qc.lib()
    ARG, NODEV = _lib.GF_ERR_ARG, _lib.GF_ERR_NO_DEVICE
    for call in (_stats, _insert):
        assert call(L, n=-1) == ARG and b"negative" in L.gf_qc_last_error()
        assert call(L, n=(1 << 38) + 1) == ARG and b"out of range" in L.gf_qc_last_error()
        assert call(L, idx=False) == ARG and b"null index" in L.gf_qc_last_error()
    assert _stats(L, table=True) == ARG and b"table" in L.gf_qc_last_error()
    assert _insert(L, hist=True) == ARG and b"table" in L.gf_qc_last_error()
    assert _stats(L, off=True) == ARG and b"offsets" in L.gf_qc_last_error()
    for hole in ("l_off", "r_off"):
        assert _insert(L, **{hole: True}) == ARG and b"offsets" in L.gf_qc_last_error(), hole
    for hole in ("bases", "quals"):
        assert _stats(L, **{hole: True}) == ARG and b"null bases or qualities" in L.gf_qc_last_error(), hole
        assert _stats(L, n=0, **{hole: True}) == NODEV   # (no records: no bases are needed)
    for hole in ("l_bases", "r_bases"):
        assert _insert(L, **{hole: True}) == ARG and b"null bases" in L.gf_qc_last_error(), hole
    # host memory: there is no CPU fallback
    for call in (_stats, _insert):
        assert call(L) == NODEV and b"no CPU fallback" in L.gf_qc_last_error()
        assert call(L, n=0) == NODEV


def test_no_cpu_fallback():
    """Host tensors (all there is without a GPU) are refused, and nothing is computed."""
    import numpy as np
    import torch
    from genefuserust_amd import Indexer
    from genefuserust_amd.fastq import FastqBatch
    ix = Indexer.from_gene_slices([b"ACGT" * 100])
    text = torch.from_numpy(np.frombuffer(b"ACGTFFFF", dtype=np.uint8).copy())
    off = torch.tensor([0, 4], dtype=torch.int64)
    batch = FastqBatch(text[:4], text[4:], off, 1, off, 0, 0)
    table = torch.zeros(read_qc.SIDE_WORDS, dtype=torch.int64)
    hist = torch.zeros(read_qc.INSERT_WORDS, dtype=torch.int64)
    with pytest.raises(_lib.GfError) as e:
        read_qc.qc_stats_device(ix, batch, table)
    assert e.value.code == _lib.GF_ERR_NO_DEVICE
    with pytest.raises(_lib.GfError) as e:
        read_qc.qc_insert_device(ix, batch, batch, hist)
    assert e.value.code == _lib.GF_ERR_NO_DEVICE
    assert int(table.sum()) == 0 and int(hist.sum()) == 0
    with pytest.raises(ValueError, match="full FASTQ cut"):
        read_qc.qc_stats_device(ix, batch._replace(qual_off=off), table)
