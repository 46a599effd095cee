"""CPU-side checks of libgfadapt.so, the adapter trimming (include/gf_adapter_trim.h): it loads next to libgfmatch.so,
exports what its header declares with the signatures adapter_trim.py binds, is bound by INTEGRATION.md, sizes its
workspace, refuses settings out of range and bad arguments before it touches a device, and has no CPU fallback."""
import ctypes as C
import os
import re
import subprocess

import pytest

from genefuserust_amd import _lib, adapter_trim
from genefuserust_amd.adapter_trim import AdapterTrim, GfAtSettings, settings_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["gf_at_last_error", "gf_at_trim_device", "gf_at_workspace_bytes"]
INT_FIELDS = ["overlap", "min_overlap", "max_diff", "diff_percent", "min_adapter", "adapter_r1_len", "adapter_r2_len"]
TRUSEQ_R1, TRUSEQ_R2 = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"


def _header() -> str:
    return open(os.path.join(ROOT, "include", "gf_adapter_trim.h")).read()


def _declarations():
    """{entry point: [parameter type, ...]} of include/gf_adapter_trim.h."""
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(gf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        out[name] = [] if params.strip() == "void" else [" ".join(p.split()[:-1]) for p in params.split(",")]
    return out


def test_header_declares_the_entry_points_and_the_settings():
    assert sorted(_declarations()) == ENTRY_POINTS
    struct = re.search(r"typedef struct gf_at_settings \{(.*?)\} gf_at_settings;", _header(), flags=re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    assert re.findall(r"int32_t (\w+);", struct) == INT_FIELDS
    assert re.findall(r"uint8_t (\w+)\[64\];", struct) == ["adapter_r1", "adapter_r2"]
    assert [f for f, _ in GfAtSettings._fields_] == INT_FIELDS + ["adapter_r1", "adapter_r2"]
    assert all(t is C.c_int32 for _, t in GfAtSettings._fields_[:7]) and C.sizeof(GfAtSettings) == 156
    assert "The settings, 156 bytes." in _header() and "The defaults: 1, 30, 5, 20, 10, 0, 0." in _header()
    s = settings_of(AdapterTrim())
    assert [getattr(s, f) for f in INT_FIELDS] == [1, 30, 5, 20, 10, 0, 0]
    s = settings_of(AdapterTrim(overlap=False, adapter_r1="illumina", adapter_r2="ACGTACGTACGT"))
    assert [getattr(s, f) for f in INT_FIELDS] == [0, 30, 5, 20, 10, 33, 12]
    assert bytes(s.adapter_r1)[:33] == TRUSEQ_R1.encode() and bytes(s.adapter_r2) == b"ACGTACGTACGT" + bytes(52)


def test_library_exports_and_signatures_match_the_header():
    L = adapter_trim.lib()
    ctype_of = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    for name, params in _declarations().items():
        assert hasattr(L, name), "libgfadapt.so does not export %s" % name
        assert getattr(L, name).argtypes == [C.c_void_p if "*" in p else ctype_of[p] for p in params], name
    assert L.gf_at_last_error.restype == C.c_char_p and L.gf_at_workspace_bytes.restype == C.c_int64
    assert len(_declarations()["gf_at_trim_device"]) == 20
    nm = subprocess.run(["nm", "-D", "--defined-only", adapter_trim.AT_LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:   # nothing but the header's functions carries the library's prefix
        exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
        assert {s for s in exported if s.startswith("gf_at_")} == set(ENTRY_POINTS)


def test_library_needs_libgfmatch_next_to_it():
    out = subprocess.run(["readelf", "-d", adapter_trim.AT_LIB_PATH], capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("readelf not available")
    assert "[libgfmatch.so]" in out.stdout and "$ORIGIN" in out.stdout


def test_integration_doc_binds_every_entry_point():
    """INTEGRATION.md's `extern "C"` block for gf_adapter_trim.h binds every function of the header, with as many
    parameters, the settings as a struct of the header's fields, and its constants are the header's."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = doc.index('extern "C" {', doc.index("pub struct gf_at_settings {"))
    block = doc[start:doc.index("}", start)]
    assert sorted(set(re.findall(r"pub fn (gf_[a-z0-9_]+)\(", block))) == ENTRY_POINTS
    for name, params in _declarations().items():
        bound = re.search(r"pub fn %s\(([^)]*)\)" % name, block).group(1)
        assert len([p for p in bound.split(",") if p.strip()]) == len(params), name
    struct = doc[doc.index("pub struct gf_at_settings {"):start]
    struct = struct[:struct.index("}")]
    assert re.findall(r"pub (\w+): i32,", struct) == INT_FIELDS
    assert re.findall(r"pub (\w+): \[u8; 64\],", struct) == ["adapter_r1", "adapter_r2"]
    defines = dict(re.findall(r"#define (GF_AT_[A-Z0-9_]+) (\d+)", _header()))
    consts = dict(re.findall(r"pub const (GF_AT_[A-Z0-9_]+): \w+ = (\d+);", doc))
    assert consts == defines and len(defines) == 7


def test_constants_are_the_bindings():
    defines = {k: int(v) for k, v in re.findall(r"#define (GF_AT_[A-Z0-9_]+) (\d+)", _header())}
    assert defines["GF_AT_READ_MAX"] == adapter_trim.READ_MAX == 512
    assert defines["GF_AT_ADAPTER_MAX"] == adapter_trim.ADAPTER_MAX == 64
    assert defines["GF_AT_TOTALS"] == adapter_trim.TOTALS == 6 == len(adapter_trim.ADAPTER_COUNTER_KEYS) + 1
    assert [defines[k] for k in ("GF_AT_UNTOUCHED", "GF_AT_BY_OVERLAP", "GF_AT_BY_SEQUENCE", "GF_AT_OVERLAP_CLEAN")] == \
        [adapter_trim.UNTOUCHED, adapter_trim.BY_OVERLAP, adapter_trim.BY_SEQUENCE, adapter_trim.OVERLAP_CLEAN] == \
        [0, 1, 2, 3]
    assert (adapter_trim.TRUSEQ_R1, adapter_trim.TRUSEQ_R2) == (TRUSEQ_R1, TRUSEQ_R2)


def test_workspace_is_monotone_in_the_record_count():
    L = adapter_trim.lib()
    counts = [0, 1, 255, 256, 257, 65536, 1 << 18, (1 << 18) + 1, 1 << 20, 20_000_000]
    w = [L.gf_at_workspace_bytes(n) for n in counts]
    assert all(a <= b for a, b in zip(w, w[1:])), w
    assert all(x >= 2 * 8 * (n // 256) for x, n in zip(w, counts))   # a sum per tile and side at the very least
    assert L.gf_at_workspace_bytes(-1) == 0


def _raw(ints, r1=b"", r2=b""):
    pad = lambda a: (C.c_uint8 * 64)(*a[:64])   # noqa: E731
    return GfAtSettings(*ints, pad(r1), pad(r2))


OK = _raw([1, 30, 5, 20, 10, 33, 33], TRUSEQ_R1.encode(), TRUSEQ_R2.encode())


def _call(L, settings=OK, idx=True, n=10, ws_bytes=1 << 20, mates=True, **null):
    """gf_at_trim_device over host memory that is never dereferenced: the checks come first."""
    buf = (C.c_char * 256)()
    dummy = C.cast(buf, C.c_void_p)
    p = lambda name, there=True: None if null.get(name) or not there else dummy   # noqa: E731
    return L.gf_at_trim_device(dummy if idx else None, None if null.get("settings_ptr") else C.byref(settings),
                               p("l_bases"), p("l_quals"), p("l_off"), p("r_bases", mates), p("r_quals", mates),
                               p("r_off", mates), n, p("ws"), ws_bytes, p("l_out_bases"), p("l_out_quals"),
                               p("l_out_off"), p("r_out_bases", mates), p("r_out_quals", mates), p("r_out_off", mates),
                               p("how"), p("totals"), None)


def test_settings_are_refused_before_anything_is_queued():
    L = adapter_trim.lib()
    a1, a2 = TRUSEQ_R1.encode(), TRUSEQ_R2.encode()
    ok = [1, 30, 5, 20, 10, 33, 33]
    change = lambda k, v: ok[:k] + [v] + ok[k + 1:]   # noqa: E731
    bad = [(change(0, 2), a1, a2), (change(0, -1), a1, a2), (change(1, 7), a1, a2), (change(1, 513), a1, a2),
           (change(2, -1), a1, a2), (change(3, -1), a1, a2), (change(3, 101), a1, a2), (change(4, 3), a1, a2),
           (change(4, 65), a1, a2), (change(5, 9), a1, a2), (change(5, 65), a1, a2), (change(6, -1), a1, a2),
           (change(6, 5), a1, a2), (change(4, 34), a1, a2),                      # an adapter shorter than min_adapter
           (ok, a1[:7] + b"N" + a1[8:], a2), (ok, a1, a2.lower()), (ok, a1[:20], a2),   # (a zero byte inside the length)
           ([0, 30, 5, 20, 10, 0, 0], b"", b"")]                                 # nothing to do
    for ints, r1, r2 in bad:
        assert _call(L, _raw(ints, r1, r2)) == _lib.GF_ERR_ARG, (ints, r1, r2)
        assert b"settings: " in L.gf_at_last_error(), ints
    assert b"nothing to do" in L.gf_at_last_error()
    assert _call(L, settings_ptr=True) == _lib.GF_ERR_ARG and b"null settings" in L.gf_at_last_error()
    # single-end input needs adapter_r1
    for ints, r1, r2 in (([1, 30, 5, 20, 10, 0, 0], b"", b""), ([1, 30, 5, 20, 10, 0, 33], b"", a2)):
        assert _call(L, _raw(ints, r1, r2), mates=False) == _lib.GF_ERR_ARG and b"single-end" in L.gf_at_last_error()
        assert _call(L, _raw(ints, r1, r2)) == _lib.GF_ERR_NO_DEVICE
    # the edges of the ranges are taken: the call gets as far as asking where the offsets live
    for ints, r1, r2 in (([1, 8, 0, 0, 4, 4, 0], b"ACGT", b""), ([0, 512, 2 ** 31 - 1, 100, 64, 64, 64], a1 + a1[:31], a2 + a2[:31]),
                         ([1, 30, 5, 20, 10, 0, 0], b"", b"")):
        assert _call(L, _raw(ints, r1, r2)) == _lib.GF_ERR_NO_DEVICE, ints
    # AdapterTrim refuses the same
    for kw in (dict(overlap=2), dict(overlap=None), dict(min_overlap=7), dict(min_overlap=513), dict(max_diff=-1),
               dict(diff_percent=101), dict(diff_percent=-1), dict(min_adapter=3), dict(min_adapter=65),
               dict(adapter_r1="ACGTACGTA"), dict(adapter_r2="A" * 65), dict(adapter_r1="ACGTNACGTACGT"),
               dict(adapter_r2=TRUSEQ_R2.lower()), dict(adapter_r1=b"ACGTACGTACGT"), dict(adapter_r1=None),
               dict(adapter_r1="illumina", min_adapter=34), dict(overlap=False), dict(min_overlap=30.0),
               dict(max_diff=True)):
        with pytest.raises(ValueError, match="AdapterTrim"):
            AdapterTrim(**kw)
    AdapterTrim(False, "ACGT", "", 8, 0, 0, 4)
    assert AdapterTrim(adapter_r1="illumina", adapter_r2="illumina") == AdapterTrim(adapter_r1=TRUSEQ_R1, adapter_r2=TRUSEQ_R2)


def test_argument_errors_without_a_device():
    L = adapter_trim.lib()
    ARG, CAP, NODEV = _lib.GF_ERR_ARG, _lib.GF_ERR_CAPACITY, _lib.GF_ERR_NO_DEVICE
    assert _call(L, n=-1) == ARG and b"negative" in L.gf_at_last_error()
    assert _call(L, ws_bytes=-5) == ARG and b"negative" in L.gf_at_last_error()
    assert _call(L, idx=False) == ARG and b"null index" in L.gf_at_last_error()
    assert _call(L, totals=True) == ARG and b"totals" in L.gf_at_last_error()
    for hole in ("l_off", "l_out_off"):
        assert _call(L, **{hole: True}) == ARG and b"offsets" in L.gf_at_last_error(), hole
    for hole in ("l_bases", "l_quals"):
        assert _call(L, **{hole: True}) == ARG and b"null bases or qualities" in L.gf_at_last_error(), hole
    for hole in ("l_out_bases", "l_out_quals", "r_out_bases", "r_out_quals"):
        assert _call(L, **{hole: True}) == ARG and b"output" in L.gf_at_last_error(), hole
    assert _call(L, how=True) == ARG and b"null how" in L.gf_at_last_error()
    for hole in ("r_bases", "r_quals", "r_off"):   # mates: all three pointers, or none
        assert _call(L, **{hole: True}) == ARG and b"mates" in L.gf_at_last_error(), hole
    assert _call(L, r_out_off=True) == ARG
    assert _call(L, ws_bytes=8) == CAP and b"gf_at_workspace_bytes" in L.gf_at_last_error()
    assert _call(L, ws=True) == CAP
    # host memory: there is no CPU fallback
    assert _call(L) == NODEV and b"no CPU fallback" in L.gf_at_last_error()
    assert _call(L, mates=False) == NODEV and _call(L, n=0) == NODEV


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
        adapter_trim.trim_adapters_device(ix, AdapterTrim(), batch, batch)
    assert e.value.code == _lib.GF_ERR_NO_DEVICE
    with pytest.raises(ValueError, match="full FASTQ cut"):
        adapter_trim.trim_adapters_device(ix, AdapterTrim(), batch._replace(qual_off=off), batch)
    with pytest.raises(ValueError, match="adapter_r1"):
        adapter_trim.trim_adapters_device(ix, AdapterTrim(), batch)
    with pytest.raises(ValueError):
        adapter_trim.trim_adapters_device(ix, None, batch, batch)
