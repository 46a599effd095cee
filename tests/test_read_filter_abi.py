"""CPU-side checks of libgfprep.so, the read filter (include/gf_read_filter.h): it loads next to libgfmatch.so, exports
what its header declares with the signatures read_filter.py binds, is bound by INTEGRATION.md, sizes its workspace,
refuses settings out of range and bad arguments before it touches a device, and has no CPU fallback."""
import ctypes as C
import os
import re
import subprocess

import pytest

from genefuserust_amd import _lib, read_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["gf_pp_filter_device", "gf_pp_last_error", "gf_pp_workspace_bytes"]
FIELDS = ["poly_g_min", "cut_tail_window", "cut_tail_mean", "length_required", "n_base_limit", "qualified_phred",
          "unqualified_percent"]


def _header() -> str:
    return open(os.path.join(ROOT, "include", "gf_read_filter.h")).read()


def _declarations():
    """{entry point: [parameter type, ...]} of include/gf_read_filter.h."""
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(gf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        out[name] = [] if params.strip() == "void" else [" ".join(p.split()[:-1]) for p in params.split(",")]
    return out


def test_header_declares_the_entry_points_and_the_settings():
    assert sorted(_declarations()) == ENTRY_POINTS
    struct = re.search(r"typedef struct gf_pp_settings \{(.*?)\} gf_pp_settings;", _header(), flags=re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    assert re.findall(r"int32_t (\w+);", struct) == FIELDS
    assert [f for f, _ in read_filter.GfPpSettings._fields_] == FIELDS
    assert all(t is C.c_int32 for _, t in read_filter.GfPpSettings._fields_) and C.sizeof(read_filter.GfPpSettings) == 28
    defaults = read_filter.ReadFilter()
    assert [getattr(defaults, f) for f in FIELDS] == [10, 0, 20, 15, 5, 15, 40]
    assert "The defaults: 10, 0, 20, 15, 5, 15, 40." in _header()


def test_library_exports_and_signatures_match_the_header():
    L = read_filter.lib()
    ctype_of = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    for name, params in _declarations().items():
        assert hasattr(L, name), "libgfprep.so does not export %s" % name
        assert getattr(L, name).argtypes == [C.c_void_p if "*" in p else ctype_of[p] for p in params], name
    assert L.gf_pp_last_error.restype == C.c_char_p and L.gf_pp_workspace_bytes.restype == C.c_int64
    assert len(_declarations()["gf_pp_filter_device"]) == 20
    nm = subprocess.run(["nm", "-D", "--defined-only", read_filter.PP_LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:   # nothing but the header's functions carries the library's prefix
        exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
        assert {s for s in exported if s.startswith("gf_pp_")} == set(ENTRY_POINTS)


def test_library_needs_libgfmatch_next_to_it():
    out = subprocess.run(["readelf", "-d", read_filter.PP_LIB_PATH], capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("readelf not available")
    assert "[libgfmatch.so]" in out.stdout and "$ORIGIN" in out.stdout


def test_integration_doc_binds_every_entry_point():
    """INTEGRATION.md's `extern "C"` block for gf_read_filter.h binds every function of the header, with as many
    parameters, the settings as a struct of the header's fields, and its constants are the header's."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = doc.index('extern "C" {', doc.index("pub struct gf_pp_settings {"))
    block = doc[start:doc.index("}", start)]
    assert sorted(set(re.findall(r"pub fn (gf_[a-z0-9_]+)\(", block))) == ENTRY_POINTS
    for name, params in _declarations().items():
        bound = re.search(r"pub fn %s\(([^)]*)\)" % name, block).group(1)
        assert len([p for p in bound.split(",") if p.strip()]) == len(params), name
    struct = doc[doc.index("pub struct gf_pp_settings {"):start]
    assert re.findall(r"pub (\w+): i32,", struct[:struct.index("}")]) == FIELDS
    defines = dict(re.findall(r"#define (GF_PP_[A-Z0-9_]+) (\d+)", _header()))
    consts = dict(re.findall(r"pub const (GF_PP_[A-Z0-9_]+): \w+ = (\d+);", doc))
    assert consts == defines and len(defines) == 8


def test_constants_are_the_bindings():
    defines = {k: int(v) for k, v in re.findall(r"#define (GF_PP_[A-Z0-9_]+) (\d+)", _header())}
    assert defines["GF_PP_WINDOW_MAX"] == read_filter.WINDOW_MAX == 64
    assert defines["GF_PP_PHRED_MAX"] == read_filter.PHRED_MAX == 93
    assert defines["GF_PP_TOTALS"] == 8 == len(read_filter.COUNTER_KEYS) + 1
    assert [defines[k] for k in ("GF_PP_KEPT", "GF_PP_TOO_SHORT", "GF_PP_TOO_MANY_N", "GF_PP_LOW_QUALITY",
                                 "GF_PP_MATE_FAILED")] == [0, 1, 2, 3, 4]


def test_workspace_is_monotone_in_the_record_count():
    L = read_filter.lib()
    counts = [0, 1, 255, 256, 257, 65536, 1 << 18, (1 << 18) + 1, 1 << 20, 20_000_000]
    w = [L.gf_pp_workspace_bytes(n) for n in counts]
    assert all(a <= b for a, b in zip(w, w[1:])), w
    assert all(x >= 2 * 8 * (n // 256) for x, n in zip(w, counts))   # a sum per tile and side at the very least
    assert L.gf_pp_workspace_bytes(-1) == 0


def _call(L, settings=None, idx=True, n=10, ws_bytes=1 << 20, mates=False, **null):
    """gf_pp_filter_device over host memory that is never dereferenced: the checks come first."""
    buf = (C.c_char * 256)()
    dummy = C.cast(buf, C.c_void_p)
    s = read_filter.GfPpSettings(*(settings if settings is not None else (10, 0, 20, 15, 5, 15, 40)))
    p = lambda name, there=True: None if null.get(name) or not there else dummy   # noqa: E731
    return L.gf_pp_filter_device(dummy if idx else None, None if null.get("settings_ptr") else C.byref(s), p("l_bases"),
                                 p("l_quals"), p("l_off"), p("r_bases", mates), p("r_quals", mates), p("r_off", mates), n,
                                 p("ws"), ws_bytes, p("l_out_bases"), p("l_out_quals"), p("l_out_off"),
                                 p("r_out_bases", mates), p("r_out_quals", mates), p("r_out_off", mates), p("reasons"),
                                 p("totals"), None)


def test_settings_out_of_range_are_refused_before_anything_is_queued():
    L = read_filter.lib()
    ok = [10, 0, 20, 15, 5, 15, 40]
    bad = [ok[:k] + [-1] + ok[k + 1:] for k in range(7)]
    bad += [[10, 65, 20, 15, 5, 15, 40], [10, 4, 94, 15, 5, 15, 40], [10, 0, 20, 15, 5, 94, 40],
            [10, 0, 20, 15, 5, 15, 101], [4097, 0, 20, 15, 5, 15, 40], [10, 0, 20, 4097, 5, 15, 40]]
    for s in bad:
        assert _call(L, s) == _lib.GF_ERR_ARG, s
        assert b"settings: " in L.gf_pp_last_error(), s
    assert b"length_required" in L.gf_pp_last_error()
    assert _call(L, settings_ptr=True) == _lib.GF_ERR_ARG and b"null settings" in L.gf_pp_last_error()
    # the largest values are taken: the call gets as far as asking where the offsets live
    for s in ([4096, 64, 93, 4096, 2 ** 31 - 1, 93, 100], [0] * 7):
        assert _call(L, s) == _lib.GF_ERR_NO_DEVICE, s
    # ReadFilter refuses the same
    for s in bad:
        with pytest.raises(ValueError, match="ReadFilter"):
            read_filter.ReadFilter(*s)
    read_filter.ReadFilter(4096, 64, 93, 4096, 2 ** 31 - 1, 93, 100)


def test_argument_errors_without_a_device():
    L = read_filter.lib()
    ARG, CAP, NODEV = _lib.GF_ERR_ARG, _lib.GF_ERR_CAPACITY, _lib.GF_ERR_NO_DEVICE
    assert _call(L, n=-1) == ARG and b"negative" in L.gf_pp_last_error()
    assert _call(L, ws_bytes=-5) == ARG and b"negative" in L.gf_pp_last_error()
    assert _call(L, idx=False) == ARG and b"null index" in L.gf_pp_last_error()
    assert _call(L, totals=True) == ARG and b"totals" in L.gf_pp_last_error()
    for hole in ("l_off", "l_out_off"):
        assert _call(L, **{hole: True}) == ARG and b"offsets" in L.gf_pp_last_error(), hole
    for hole in ("l_bases", "l_quals"):
        assert _call(L, **{hole: True}) == ARG and b"null bases or qualities" in L.gf_pp_last_error(), hole
    for hole in ("l_out_bases", "l_out_quals"):
        assert _call(L, **{hole: True}) == ARG and b"output" in L.gf_pp_last_error(), hole
    assert _call(L, reasons=True) == ARG and b"reasons" in L.gf_pp_last_error()
    for hole in ("r_bases", "r_quals", "r_off"):   # mates: all three pointers, or none
        assert _call(L, mates=True, **{hole: True}) == ARG and b"mates" in L.gf_pp_last_error(), hole
    assert _call(L, mates=True, r_out_off=True) == ARG
    assert _call(L, mates=True, r_out_quals=True) == ARG and b"output" in L.gf_pp_last_error()
    assert _call(L, ws_bytes=8) == CAP and b"gf_pp_workspace_bytes" in L.gf_pp_last_error()
    assert _call(L, ws=True) == CAP
    # host memory: there is no CPU fallback
    assert _call(L) == NODEV and b"no CPU fallback" in L.gf_pp_last_error()
    assert _call(L, mates=True) == NODEV and _call(L, n=0) == NODEV


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
    with pytest.raises(_lib.GfError) as e:
        read_filter.filter_reads_device(ix, read_filter.ReadFilter(), batch)
    assert e.value.code == _lib.GF_ERR_NO_DEVICE
    with pytest.raises(ValueError, match="full FASTQ cut"):
        read_filter.filter_reads_device(ix, read_filter.ReadFilter(), batch._replace(qual_off=off))
    with pytest.raises(ValueError):
        read_filter.filter_reads_device(ix, None, batch)
