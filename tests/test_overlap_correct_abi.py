"""CPU-side checks of libgfcorrect.so, the correction inside the pair overlap (include/gf_overlap_correct.h): it loads
next to libgfmatch.so, exports what its header declares with the signatures overlap_correct.py binds, is bound by
INTEGRATION.md, refuses settings out of range and bad arguments before it touches a device, and has no CPU fallback."""
import ctypes as C
import os
import re
import subprocess

import pytest

from genefuserust_amd import _lib, overlap_correct
from genefuserust_amd.overlap_correct import GfOcSettings, OverlapCorrect, settings_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["gf_oc_correct_device", "gf_oc_last_error"]
FIELDS = ["min_overlap", "max_diff", "diff_percent", "good_phred", "bad_phred"]


def _header() -> str:
    return open(os.path.join(ROOT, "include", "gf_overlap_correct.h")).read()


def _declarations():
    """{entry point: [parameter type, ...]} of include/gf_overlap_correct.h."""
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(gf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        out[name] = [] if params.strip() == "void" else [" ".join(p.split()[:-1]) for p in params.split(",")]
    return out


def test_header_declares_the_entry_points_and_the_settings():
    assert sorted(_declarations()) == ENTRY_POINTS
    struct = re.search(r"typedef struct gf_oc_settings \{(.*?)\} gf_oc_settings;", _header(), flags=re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    assert re.findall(r"int32_t (\w+);", struct) == FIELDS
    assert [f for f, _ in GfOcSettings._fields_] == FIELDS
    assert all(t is C.c_int32 for _, t in GfOcSettings._fields_) and C.sizeof(GfOcSettings) == 20
    assert "The settings, 20 bytes." in _header() and "The defaults: 30, 5, 20, 30, 15" in _header()
    s = settings_of(OverlapCorrect())
    assert [getattr(s, f) for f in FIELDS] == [30, 5, 20, 30, 15]
    assert (ord("?") - 33, ord("0") - 33) == (30, 15)   # fast_merge's two quality letters
    s = settings_of(OverlapCorrect(8, 0, 100, 93, 0))
    assert [getattr(s, f) for f in FIELDS] == [8, 0, 100, 93, 0]


def test_library_exports_and_signatures_match_the_header():
    L = overlap_correct.lib()
    ctype_of = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    for name, params in _declarations().items():
        assert hasattr(L, name), "libgfcorrect.so does not export %s" % name
        assert getattr(L, name).argtypes == [C.c_void_p if "*" in p else ctype_of[p] for p in params], name
    assert L.gf_oc_last_error.restype == C.c_char_p and L.gf_oc_correct_device.restype == C.c_int
    assert len(_declarations()["gf_oc_correct_device"]) == 13
    nm = subprocess.run(["nm", "-D", "--defined-only", overlap_correct.OC_LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:   # nothing but the header's functions carries the library's prefix
        exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
        assert {s for s in exported if s.startswith("gf_oc_")} == set(ENTRY_POINTS)
        assert not {s for s in exported if s.startswith("gf_at_")}   # the search is included, not exported again


def test_library_needs_libgfmatch_next_to_it():
    out = subprocess.run(["readelf", "-d", overlap_correct.OC_LIB_PATH], capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("readelf not available")
    assert "[libgfmatch.so]" in out.stdout and "$ORIGIN" in out.stdout


def test_the_build_names_the_library():
    makefile = open(os.path.join(ROOT, "genefuserust_amd", "scan_csrc", "Makefile")).read()
    assert "../libgfcorrect.so: gf_overlap_correct.hip $(HDRS) ../libgfmatch.so" in makefile
    for target in ("all", "clean", "resource-usage"):
        rule = re.search(r"^%s:.*?(?=^\S|\Z)" % target, makefile, flags=re.M | re.S).group(0)
        assert ("libgfcorrect.so" if target != "resource-usage" else "gf_overlap_correct.hip") in rule, target
    assert "libgfcorrect.so" in makefile[:makefile.index("HIPCC ?=")]          # the header comment
    assert "libgfcorrect.so" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    for name in ("gf_overlap_correct.hip", "gf_oc_core.h", "gf_oc_kernels.h"):
        assert os.path.exists(os.path.join(ROOT, "genefuserust_amd", "scan_csrc", name)), name


def test_integration_doc_binds_every_entry_point():
    """INTEGRATION.md's `extern "C"` block for gf_overlap_correct.h binds every function of the header, with as many
    parameters, the settings as a struct of the header's fields, and its constants are the header's."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = doc.index('extern "C" {', doc.index("pub struct gf_oc_settings {"))
    block = doc[start:doc.index("}", start)]
    assert sorted(set(re.findall(r"pub fn (gf_[a-z0-9_]+)\(", block))) == ENTRY_POINTS
    for name, params in _declarations().items():
        bound = re.search(r"pub fn %s\(([^)]*)\)" % name, block).group(1)
        assert len([p for p in bound.split(",") if p.strip()]) == len(params), name
    struct = doc[doc.index("pub struct gf_oc_settings {"):start]
    struct = struct[:struct.index("}")]
    assert re.findall(r"pub (\w+): i32,", struct) == FIELDS
    defines = dict(re.findall(r"#define (GF_OC_[A-Z0-9_]+) (\d+)", _header()))
    consts = dict(re.findall(r"pub const (GF_OC_[A-Z0-9_]+): \w+ = (\d+);", doc))
    assert consts == defines and len(defines) == 2


def test_constants_are_the_bindings():
    defines = {k: int(v) for k, v in re.findall(r"#define (GF_OC_[A-Z0-9_]+) (\d+)", _header())}
    assert defines["GF_OC_TOTALS"] == overlap_correct.TOTALS == 6 == len(overlap_correct.CORRECT_COUNTER_KEYS) + 1
    assert defines["GF_OC_PHRED_MAX"] == overlap_correct.PHRED_MAX == 93
    assert overlap_correct.READ_MAX == 512
    assert overlap_correct.CORRECT_COUNTER_KEYS == ("correction_overlapping_pairs", "correction_pairs_with_diffs",
                                                    "corrected_reads", "corrected_bases", "correction_diffs_left")
    assert overlap_correct.correct_totals_counters([9, 8, 7, 6, 5, 4]) == dict(
        correction_overlapping_pairs=8, correction_pairs_with_diffs=7, corrected_reads=6, corrected_bases=5,
        correction_diffs_left=4)
    import genefuserust_amd
    assert genefuserust_amd.OverlapCorrect is OverlapCorrect
    assert genefuserust_amd.correct_overlaps_device is overlap_correct.correct_overlaps_device


OK = GfOcSettings(30, 5, 20, 30, 15)


def _call(L, settings=OK, idx=True, n=10, mates=True, **null):
    """gf_oc_correct_device over host memory that is never dereferenced: the checks come first."""
    buf = (C.c_char * 256)()
    dummy = C.cast(buf, C.c_void_p)
    p = lambda name, there=True: None if null.get(name) or not there else dummy   # noqa: E731
    return L.gf_oc_correct_device(dummy if idx else None, None if null.get("settings_ptr") else C.byref(settings),
                                  p("l_bases"), p("l_quals"), p("l_off"), p("r_bases", mates), p("r_quals", mates),
                                  p("r_off", mates), n, p("insert"), p("fixed"), p("totals"), None)


def test_settings_are_refused_before_anything_is_queued():
    L = overlap_correct.lib()
    ok = [30, 5, 20, 30, 15]
    change = lambda k, v, base=ok: base[:k] + [v] + base[k + 1:]   # noqa: E731
    bad = [change(0, 7), change(0, 513), change(1, -1), change(2, -1), change(2, 101), change(3, -1), change(3, 94),
           change(4, -1), change(4, 30), change(4, 31), [30, 5, 20, 93, 94], [30, 5, 20, 0, 0]]
    for ints in bad:
        assert _call(L, GfOcSettings(*ints)) == _lib.GF_ERR_ARG, ints
        assert L.gf_oc_last_error().startswith(b"settings: "), ints
    assert _call(L, settings_ptr=True) == _lib.GF_ERR_ARG and b"null settings" in L.gf_oc_last_error()
    # the edges of the ranges are taken: the call gets as far as asking where the offsets live
    for ints in ([8, 0, 0, 1, 0], [512, 2 ** 31 - 1, 100, 93, 92], ok):
        assert _call(L, GfOcSettings(*ints)) == _lib.GF_ERR_NO_DEVICE, ints
    # OverlapCorrect refuses the same, and what is no integer
    for ints in bad:
        with pytest.raises(ValueError, match="OverlapCorrect"):
            OverlapCorrect(*ints)
    for kw in (dict(min_overlap=30.0), dict(max_diff=True), dict(good_phred="30"), dict(bad_phred=None),
               dict(max_diff=2 ** 31)):
        with pytest.raises(ValueError, match="OverlapCorrect"):
            OverlapCorrect(**kw)
    OverlapCorrect(8, 0, 0, 1, 0)
    OverlapCorrect(512, 2 ** 31 - 1, 100, 93, 92)
    with pytest.raises(Exception):   # frozen
        OverlapCorrect().good_phred = 20
    assert overlap_correct.need_overlap_correct(None) is None
    assert overlap_correct.need_overlap_correct(OverlapCorrect(max_diff=3)) == OverlapCorrect(max_diff=3)
    for wrong in (True, 1, "on", dict(), OverlapCorrect):
        with pytest.raises(ValueError, match="overlap_correct"):
            overlap_correct.need_overlap_correct(wrong)
    with pytest.raises(ValueError, match="pairs"):
        overlap_correct.need_pairs(OverlapCorrect(), False)
    assert overlap_correct.need_pairs(None, False) is None and overlap_correct.need_pairs(OverlapCorrect(), True)


def test_argument_errors_without_a_device():
    L = overlap_correct.lib()
    ARG, NODEV = _lib.GF_ERR_ARG, _lib.GF_ERR_NO_DEVICE
    assert _call(L, n=-1) == ARG and b"negative" in L.gf_oc_last_error()
    assert _call(L, idx=False) == ARG and b"null index" in L.gf_oc_last_error()
    assert _call(L, totals=True) == ARG and b"totals" in L.gf_oc_last_error()
    assert _call(L, l_off=True) == ARG and b"offsets" in L.gf_oc_last_error()
    for hole in ("l_bases", "l_quals"):
        assert _call(L, **{hole: True}) == ARG and b"null bases or qualities" in L.gf_oc_last_error(), hole
    for hole in ("r_bases", "r_quals", "r_off"):   # mates: all three pointers
        assert _call(L, **{hole: True}) == ARG and b"some of the mates' pointers" in L.gf_oc_last_error(), hole
    assert _call(L, mates=False) == ARG and b"pairs" in L.gf_oc_last_error()   # the call is for pairs
    # host memory: there is no CPU fallback; insert and fixed may be null
    assert _call(L) == NODEV and b"no CPU fallback" in L.gf_oc_last_error()
    assert _call(L, insert=True, fixed=True) == NODEV and _call(L, n=0) == NODEV


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
    for inplace in (False, True):
        with pytest.raises(_lib.GfError) as e:
            overlap_correct.correct_overlaps_device(ix, OverlapCorrect(), batch, batch, inplace=inplace)
        assert e.value.code == _lib.GF_ERR_NO_DEVICE
    assert bytes(text.numpy()) == b"ACGTFFFF"
    with pytest.raises(ValueError, match="full FASTQ cut"):
        overlap_correct.correct_overlaps_device(ix, OverlapCorrect(), batch._replace(qual_off=off), batch)
    with pytest.raises(ValueError, match="pairs"):
        overlap_correct.correct_overlaps_device(ix, OverlapCorrect(), batch, None)
    with pytest.raises(ValueError):
        overlap_correct.correct_overlaps_device(ix, None, batch, batch)
