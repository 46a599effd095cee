"""CPU-side checks of libgfdedup.so, the duplicate removal (include/gf_dedup.h): it loads next to libgfmatch.so, exports
what its header declares with the signatures dedup.py binds, is bound by INTEGRATION.md, its constants are the
bindings', it refuses bad arguments before it touches a device, and has no CPU fallback."""
import ctypes as C
import os
import re
import subprocess

import pytest

from genefuserust_amd import _lib, dedup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["gf_dd_histogram_device", "gf_dd_insert_device", "gf_dd_keys_device", "gf_dd_last_error",
                "gf_dd_rehash_device", "gf_dd_remove_device", "gf_dd_workspace_bytes"]
PARAMETERS = {"gf_dd_keys_device": 8, "gf_dd_insert_device": 11, "gf_dd_workspace_bytes": 1, "gf_dd_remove_device": 22,
              "gf_dd_rehash_device": 10, "gf_dd_histogram_device": 6, "gf_dd_last_error": 0}


def _header() -> str:
    return open(os.path.join(ROOT, "include", "gf_dedup.h")).read()


def _declarations():
    """{entry point: [parameter type, ...]} of include/gf_dedup.h."""
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(gf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        out[name] = [] if params.strip() == "void" else [" ".join(p.split()[:-1]) for p in params.split(",")]
    return out


def _defines() -> dict:
    return {k: int(v) for k, v in re.findall(r"#define (GF_DD_[A-Z0-9_]+) (\d+)", _header())}


def test_header_declares_the_entry_points_and_states_the_predicate():
    d = _declarations()
    assert sorted(d) == ENTRY_POINTS and {k: len(v) for k, v in d.items()} == PARAMETERS
    for phrase in ("fold(c) = c & 0xDF", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "0x9E3779B97F4A7C15",
                   "K = mix(H(r1) + mix(H(r2) + 1))", "A K of 0 becomes 1", "0xab0fcab10dd0c6f9", "0xade372bd9e169438",
                   "lowest global", "n^2 / 2^65", "INT64_MAX", "not\n * contract", "no CPU fallback"):
        assert phrase in _header(), phrase


def test_library_exports_and_signatures_match_the_header():
    L = dedup.lib()
    ctype_of = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    for name, params in _declarations().items():
        assert hasattr(L, name), "libgfdedup.so does not export %s" % name
        assert getattr(L, name).argtypes == [C.c_void_p if "*" in p else ctype_of[p] for p in params], name
    assert L.gf_dd_last_error.restype == C.c_char_p and L.gf_dd_workspace_bytes.restype == C.c_int64
    for name in ENTRY_POINTS:
        if name.endswith("_device"):
            assert getattr(L, name).restype == C.c_int
    nm = subprocess.run(["nm", "-D", "--defined-only", dedup.DD_LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:   # nothing but the header's functions carries the library's prefix
        exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
        assert {s for s in exported if s.startswith("gf_dd_")} == set(ENTRY_POINTS)


def test_library_needs_libgfmatch_next_to_it():
    out = subprocess.run(["readelf", "-d", dedup.DD_LIB_PATH], capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("readelf not available")
    assert "[libgfmatch.so]" in out.stdout and "$ORIGIN" in out.stdout


def test_makefile_builds_the_library_with_the_others():
    mk = open(os.path.join(ROOT, "genefuserust_amd", "scan_csrc", "Makefile")).read()
    for target in ("all:", "resource-usage:", "\trm -f"):
        line = next(x for x in mk.splitlines() if x.startswith(target))
        assert "gfdedup" in line or "gf_dedup.hip" in line, target
    assert "../libgfdedup.so: gf_dedup.hip $(HDRS) ../libgfmatch.so" in mk
    assert "-c -o /dev/null gf_dedup.hip" in mk and "libgfdedup.so" in mk.split("HIPCC ?=")[0]
    assert "libgfdedup.so" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_integration_doc_binds_every_entry_point():
    """INTEGRATION.md's `extern "C"` block for gf_dedup.h binds every function of the header, with as many parameters,
    and its constants are the header's."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = doc.index('extern "C" {', doc.index("src/gfdedup_sys.rs"))
    block = doc[start:doc.index("\n}", start)]
    assert sorted(set(re.findall(r"pub fn (gf_[a-z0-9_]+)\(", block))) == ENTRY_POINTS
    for name, params in _declarations().items():
        bound = re.search(r"pub fn %s\(([^)]*)\)" % name, block).group(1)
        assert len([p for p in bound.split(",") if p.strip()]) == len(params), name
    consts = {k: int(v) for k, v in re.findall(r"pub const (GF_DD_[A-Z0-9_]+): \w+ = (\d+);", doc)}
    assert consts == _defines() and len(consts) == 3


def test_constants_are_the_bindings_and_the_models():
    from tests import dedup_model as model
    d = _defines()
    assert d["GF_DD_LEVELS"] == dedup.LEVELS == model.LEVELS == 32
    assert d["GF_DD_TOTALS"] == dedup.TOTALS == model.TOTALS == 6
    assert d["GF_DD_MIN_SLOTS"] == dedup.MIN_SLOTS == model.MIN_SLOTS == 1024
    assert dedup.NO_INDEX == model.NO_INDEX == 2 ** 63 - 1
    assert dedup.DEDUP_COUNTER_KEYS == ("dedup_checked", "dedup_unique", "dedup_duplicates", "dedup_bases_removed")
    assert dedup.lib().gf_dd_workspace_bytes(-1) == 0
    sizes = [dedup.lib().gf_dd_workspace_bytes(n) for n in (0, 1, 256, 257, 1 << 20)]
    assert sizes == sorted(sizes) and sizes[0] > 0


def _call(L, name, idx=True, **over):
    """An entry point over host memory that is never dereferenced: the checks come first.  ``over``: a value for a
    parameter by its name in the header, None for a NULL pointer."""
    buf = (C.c_char * 256)()
    dummy = C.cast(buf, C.c_void_p)
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    params = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src).group(1).split(",")
    sizes = {"n": 10, "first_index": 0, "slots": 1024, "old_slots": 1024, "new_slots": 2048, "workspace_bytes": 1 << 20}
    args = []
    for p in params:
        pname = p.split()[-1].lstrip("*")
        if pname in over:
            args.append(over[pname])
        elif pname == "idx":
            args.append(dummy if idx else None)
        elif pname == "stream":
            args.append(None)
        elif "*" in p:
            args.append(dummy)
        else:
            args.append(sizes[pname])
    return getattr(L, name)(*args)


DEVICE_CALLS = [n for n in ENTRY_POINTS if n.endswith("_device")]


def test_argument_errors_without_a_device():
    L = dedup.lib()
    ARG, NODEV, CAP = _lib.GF_ERR_ARG, _lib.GF_ERR_NO_DEVICE, _lib.GF_ERR_CAPACITY
    err = L.gf_dd_last_error
    for name in DEVICE_CALLS:
        assert _call(L, name, idx=False) == ARG and b"null index" in err(), name
        assert _call(L, name) == NODEV and b"no CPU fallback" in err(), name   # host memory
    for name in ("gf_dd_keys_device", "gf_dd_insert_device", "gf_dd_remove_device"):
        assert _call(L, name, n=-1) == ARG and b"negative" in err(), name
        assert _call(L, name, n=(1 << 38) + 1) == ARG and b"out of range" in err(), name
    # the table: slots a power of two of at least 1024, a rehash only grows, no NULL array but count
    for name, key in (("gf_dd_insert_device", "slots"), ("gf_dd_histogram_device", "slots"),
                      ("gf_dd_rehash_device", "old_slots"), ("gf_dd_rehash_device", "new_slots")):
        for bad in (0, -1024, 512, 1023, 1025, 1536, 3 << 20):
            assert _call(L, name, **{key: bad}) == ARG and b"power of two" in err(), (name, bad)
    for old, new in ((2048, 1024), (1024, 1024), (1 << 20, 1 << 19)):
        assert _call(L, "gf_dd_rehash_device", old_slots=old, new_slots=new) == ARG and b"only grows" in err()
    for name, holes in (("gf_dd_insert_device", ("d_keys", "d_first")), ("gf_dd_histogram_device", ("d_keys", "d_count")),
                        ("gf_dd_rehash_device", ("d_old_keys", "d_old_first", "d_new_keys", "d_new_first")),
                        ("gf_dd_remove_device", ("d_first",))):
        for hole in holes:
            assert _call(L, name, **{hole: None}) == ARG and b"null table" in err(), (name, hole)
    assert _call(L, "gf_dd_insert_device", d_count=None) == NODEV          # count may be NULL
    assert _call(L, "gf_dd_rehash_device", d_old_count=None, d_new_count=None) == NODEV
    for name in ("gf_dd_insert_device", "gf_dd_remove_device"):
        assert _call(L, name, first_index=-1) == ARG and b"first_index" in err(), name
        assert _call(L, name, first_index=2 ** 63 - 5) == ARG and b"first_index" in err(), name
        assert _call(L, name, d_totals=None) == ARG and b"totals" in err(), name
    # the records
    assert _call(L, "gf_dd_keys_device", d_l_off=None) == ARG and b"offsets" in err()
    assert _call(L, "gf_dd_keys_device", d_r_off=None) == ARG and b"offsets" in err()
    assert _call(L, "gf_dd_keys_device", d_l_bases=None) == ARG and b"null bases" in err()
    assert _call(L, "gf_dd_keys_device", d_rec_keys=None) == ARG and b"record keys" in err()
    assert _call(L, "gf_dd_keys_device", d_r_bases=None, d_r_off=None) == NODEV      # single-end
    assert _call(L, "gf_dd_keys_device", n=0, d_l_bases=None, d_rec_keys=None) == NODEV
    assert _call(L, "gf_dd_insert_device", d_rec_keys=None) == ARG and b"record keys" in err()
    assert _call(L, "gf_dd_insert_device", d_rec_slot=None) == ARG and b"slots" in err()
    assert _call(L, "gf_dd_histogram_device", d_hist=None) == ARG and b"histogram" in err()
    for hole in ("d_l_off", "d_l_out_off", "d_r_out_off"):
        assert _call(L, "gf_dd_remove_device", **{hole: None}) == ARG and b"offsets" in err(), hole
    for hole in ("d_r_bases", "d_r_quals", "d_r_off"):
        assert _call(L, "gf_dd_remove_device", **{hole: None}) == ARG and b"mates" in err(), hole
    for hole in ("d_l_bases", "d_l_quals"):
        assert _call(L, "gf_dd_remove_device", **{hole: None}) == ARG and b"null bases or qualities" in err(), hole
    for hole in ("d_l_out_bases", "d_r_out_quals"):
        assert _call(L, "gf_dd_remove_device", **{hole: None}) == ARG and b"output" in err(), hole
    for hole in ("d_rec_slot", "d_dup"):
        assert _call(L, "gf_dd_remove_device", **{hole: None}) == ARG and b"record slots" in err(), hole
    assert _call(L, "gf_dd_remove_device", workspace_bytes=-1) == ARG and b"negative" in err()
    assert _call(L, "gf_dd_remove_device", workspace_bytes=16) == CAP and b"gf_dd_workspace_bytes" in err()
    assert _call(L, "gf_dd_remove_device", d_workspace=None) == CAP


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
    table = dedup.empty_table(1024, "cpu")
    totals = torch.zeros(dedup.TOTALS, dtype=torch.int64)
    calls = (lambda: dedup.keys_device(ix, batch),
             lambda: dedup.insert_device(ix, torch.ones(1, dtype=torch.int64), 0, table, totals),
             lambda: dedup.remove_device(ix, torch.zeros(1, dtype=torch.int64), 0, table, totals, batch),
             lambda: dedup.rehash_device(ix, table, dedup.empty_table(2048, "cpu")),
             lambda: dedup.histogram_device(ix, table, torch.zeros(dedup.LEVELS, dtype=torch.int64)))
    for call in calls:
        with pytest.raises(_lib.GfError) as e:
            call()
        assert e.value.code == _lib.GF_ERR_NO_DEVICE
    assert int(totals.sum()) == 0 and int(table.keys.sum()) == 0
    with pytest.raises(ValueError, match="full FASTQ cut"):
        dedup.remove_device(ix, torch.zeros(1, dtype=torch.int64), 0, table, totals, batch._replace(qual_off=off))
