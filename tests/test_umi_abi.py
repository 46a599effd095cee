"""CPU-side checks of libgfumi.so, the UMI calls (include/gf_umi.h): it loads next to libgfmatch.so, exports what its
header declares with the signatures umi.py binds, is bound by INTEGRATION.md, its constants are the bindings', it
refuses bad settings and arguments before it touches a device, and has no CPU fallback."""
import ctypes as C
import os
import re
import subprocess

import pytest

from genefuserust_amd import _lib, umi
from tests import umi_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["gf_um_cut_device", "gf_um_last_error", "gf_um_mix_keys_device", "gf_um_names_device",
                "gf_um_workspace_bytes"]
PARAMETERS = {"gf_um_cut_device": 20, "gf_um_names_device": 9, "gf_um_mix_keys_device": 5, "gf_um_workspace_bytes": 1,
              "gf_um_last_error": 0}


def _header() -> str:
    return open(os.path.join(ROOT, "include", "gf_umi.h")).read()


def _declarations():
    """{entry point: [parameter type, ...]} of include/gf_umi.h."""
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(gf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        out[name] = [] if params.strip() == "void" else [" ".join(p.split()[:-1]) for p in params.split(",")]
    return out


def _defines() -> dict:
    return {k: int(v) for k, v in re.findall(r"#define (GF_UM_[A-Z0-9_]+) (\d+)", _header())}


def test_header_declares_the_entry_points_and_states_the_predicate():
    d = _declarations()
    assert sorted(d) == ENTRY_POINTS and {k: len(v) for k, v in d.items()} == PARAMETERS
    flat = " ".join(_header().replace(" * ", " ").split())
    for phrase in ("c = length + skip", "U = mix(H(u1) + mix(H(u2) + 1))", "A U of 0 becomes 1", "K' = mix(K + mix(U + 2))",
                   "K == 0 stays 0", '"ACGTNacgtn+_"', "One trailing '\\r' is stripped", "first space or tab",
                   "0x1d189c7f508326f9", "0x8a0ec19742ea7304", "0xdecfd2a34e770449", "0xff1a16f0056acf7f",
                   "0xf6e69183b4f4f21c", "0xc7033d0180ee6594", "no CPU fallback", "up to 15 bytes", "ADDED into"):
        assert phrase in flat, phrase
    assert '#include "gf_dd_core.h"' in open(os.path.join(ROOT, "genefuserust_amd", "scan_csrc", "gf_um_core.h")).read()


def test_library_exports_and_signatures_match_the_header():
    L = umi.lib()
    ctype_of = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    for name, params in _declarations().items():
        assert hasattr(L, name), "libgfumi.so does not export %s" % name
        assert getattr(L, name).argtypes == [C.c_void_p if "*" in p else ctype_of[p] for p in params], name
    assert L.gf_um_last_error.restype == C.c_char_p and L.gf_um_workspace_bytes.restype == C.c_int64
    for name in ENTRY_POINTS:
        if name.endswith("_device"):
            assert getattr(L, name).restype == C.c_int
    nm = subprocess.run(["nm", "-D", "--defined-only", umi.UM_LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:   # nothing but the header's functions carries the library's prefix
        exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
        assert {s for s in exported if s.startswith("gf_um_")} == set(ENTRY_POINTS)
        assert not {s for s in exported if s.startswith("gf_dd_")}      # libgfdedup.so's calls stay its own


def test_library_needs_libgfmatch_next_to_it():
    out = subprocess.run(["readelf", "-d", umi.UM_LIB_PATH], capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("readelf not available")
    assert "[libgfmatch.so]" in out.stdout and "$ORIGIN" in out.stdout and "libgfdedup" not in out.stdout


def test_makefile_builds_the_library_with_the_others():
    mk = open(os.path.join(ROOT, "genefuserust_amd", "scan_csrc", "Makefile")).read()
    for target in ("all:", "resource-usage:", "\trm -f"):
        line = next(x for x in mk.splitlines() if x.startswith(target))
        assert "gfumi" in line or "gf_umi.hip" in line, target
    assert "../libgfumi.so: gf_umi.hip $(HDRS) ../libgfmatch.so" in mk
    assert "-c -o /dev/null gf_umi.hip" in mk and "libgfumi.so" in mk.split("HIPCC ?=")[0]
    assert "libgfumi.so" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_integration_doc_binds_every_entry_point():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = doc.index('extern "C" {', doc.index("src/gfumi_sys.rs"))
    block = doc[start:doc.index("\n}", start)]
    assert sorted(set(re.findall(r"pub fn (gf_[a-z0-9_]+)\(", block))) == ENTRY_POINTS
    for name, params in _declarations().items():
        bound = re.search(r"pub fn %s\(([^)]*)\)" % name, block).group(1)
        assert len([p for p in bound.split(",") if p.strip()]) == len(params), name
    consts = {k: int(v) for k, v in re.findall(r"pub const (GF_UM_[A-Z0-9_]+): \w+ = (\d+);", doc)}
    assert consts == _defines() and len(consts) == 8


def test_constants_are_the_bindings_and_the_models():
    d = _defines()
    assert (d["GF_UM_NAME"], d["GF_UM_READ1"], d["GF_UM_READ2"], d["GF_UM_PER_READ"]) == (0, 1, 2, 3)
    assert umi.SOURCES == model.SOURCES == {"name": 0, "read1": 1, "read2": 2, "per_read": 3}
    assert d["GF_UM_MAX_LEN"] == umi.MAX_LEN == model.MAX_LEN == 32
    assert d["GF_UM_MAX_SKIP"] == umi.MAX_SKIP == model.MAX_SKIP == 32
    assert d["GF_UM_MAX_FIELD"] == umi.MAX_FIELD == model.MAX_FIELD == 64
    assert d["GF_UM_TOTALS"] == umi.TOTALS == model.TOTALS == 7
    assert C.sizeof(umi.GfUmSettings) == 12
    assert umi.lib().gf_um_workspace_bytes(-1) == 0
    sizes = [umi.lib().gf_um_workspace_bytes(n) for n in (0, 1, 255, 256, 257, 600, 1 << 20, 1 << 30)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] > sizes[0]


def _call(L, name, idx=True, settings=(1, 8, 2), **over):
    """An entry point over host memory that is never dereferenced: the checks come first.  ``over``: a value for a
    parameter by its name in the header, None for a NULL pointer."""
    buf = (C.c_char * 256)()
    dummy = C.cast(buf, C.c_void_p)
    config = None if settings is None else umi.GfUmSettings(*settings)
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    params = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src).group(1).split(",")
    sizes = {"n": 10, "workspace_bytes": 1 << 20, "text_bytes": 100, "newlines": 40}
    args = []
    for p in params:
        pname = p.split()[-1].lstrip("*")
        if pname in over:
            args.append(over[pname])
        elif pname == "idx":
            args.append(dummy if idx else None)
        elif pname == "settings":
            args.append(None if config is None else C.cast(C.pointer(config), C.c_void_p))
        elif pname == "stream":
            args.append(None)
        elif "*" in p:
            args.append(dummy)
        else:
            args.append(sizes[pname])
    return getattr(L, name)(*args)


DEVICE_CALLS = [n for n in ENTRY_POINTS if n.endswith("_device")]


def test_every_refused_setting_gives_an_argument_error_with_a_message():
    L = umi.lib()
    ARG, NODEV = _lib.GF_ERR_ARG, _lib.GF_ERR_NO_DEVICE
    err = L.gf_um_last_error
    refused = 0
    for source in (-1, 0, 1, 2, 3, 4, 99):
        for length in (-1, 0, 1, 8, 32, 33):
            for skip in (-1, 0, 2, 32, 33):
                rc = _call(L, "gf_um_cut_device", settings=(source, length, skip))
                if source in (1, 2, 3) and model.settings_ok(source, length, skip):
                    assert rc == NODEV, (source, length, skip)       # accepted: the next check is the memory's
                else:
                    refused += 1
                    assert rc == ARG and len(err()) > 10, (source, length, skip)
                    assert (b"cuts nothing" in err()) == (source == 0 and length == 0 and skip == 0)
    assert refused == 7 * 6 * 5 - 3 * 3 * 3
    # read2 with single-end input
    single = dict(d_r_bases=None, d_r_quals=None, d_r_off=None, d_r_out_bases=None, d_r_out_quals=None, d_r_out_off=None)
    assert _call(L, "gf_um_cut_device", settings=(2, 8, 0), **single) == ARG and b"read2" in err()
    assert _call(L, "gf_um_cut_device", settings=(1, 8, 0), **single) == NODEV
    assert _call(L, "gf_um_cut_device", settings=(3, 8, 0), **single) == NODEV      # per_read is read1 there
    assert _call(L, "gf_um_cut_device", settings=None) == ARG and b"settings" in err()


def test_argument_errors_without_a_device():
    L = umi.lib()
    ARG, NODEV, CAP = _lib.GF_ERR_ARG, _lib.GF_ERR_NO_DEVICE, _lib.GF_ERR_CAPACITY
    err = L.gf_um_last_error
    for name in DEVICE_CALLS:
        assert _call(L, name, idx=False) == ARG and b"null index" in err(), name
        assert _call(L, name) == NODEV and b"no CPU fallback" in err(), name   # host memory
        assert _call(L, name, n=-1) == ARG and b"negative" in err(), name
        assert _call(L, name, n=(1 << 38) + 1) == ARG and b"out of range" in err(), name
    for name in ("gf_um_cut_device", "gf_um_names_device"):
        assert _call(L, name, d_totals=None) == ARG and b"totals" in err(), name
        assert _call(L, name, d_codes=None) == ARG and b"codes" in err(), name
    for hole in ("d_l_off", "d_l_out_off", "d_r_out_off"):
        assert _call(L, "gf_um_cut_device", **{hole: None}) == ARG and b"offsets" in err(), hole
    for hole in ("d_r_bases", "d_r_quals", "d_r_off"):
        assert _call(L, "gf_um_cut_device", **{hole: None}) == ARG and b"mates" in err(), hole
    for hole in ("d_l_bases", "d_l_quals"):
        assert _call(L, "gf_um_cut_device", **{hole: None}) == ARG and b"null bases or qualities" in err(), hole
    for hole in ("d_l_out_bases", "d_r_out_quals"):
        assert _call(L, "gf_um_cut_device", **{hole: None}) == ARG and b"output" in err(), hole
    assert _call(L, "gf_um_cut_device", workspace_bytes=-1) == ARG and b"negative" in err()
    assert _call(L, "gf_um_cut_device", workspace_bytes=16) == CAP and b"gf_um_workspace_bytes" in err()
    assert _call(L, "gf_um_cut_device", d_workspace=None) == CAP
    assert _call(L, "gf_um_names_device", d_text=None) == ARG and b"text" in err()
    assert _call(L, "gf_um_names_device", d_nl_pos=None) == ARG and b"newline" in err()
    assert _call(L, "gf_um_names_device", text_bytes=-1) == ARG and b"negative" in err()
    assert _call(L, "gf_um_names_device", newlines=-1) == ARG and b"negative" in err()
    assert _call(L, "gf_um_names_device", d_text=None, text_bytes=0, d_nl_pos=None, newlines=0) == NODEV
    for hole in ("d_rec_keys", "d_codes"):
        assert _call(L, "gf_um_mix_keys_device", **{hole: None}) == ARG and b"record keys or codes" in err(), hole
    assert _call(L, "gf_um_mix_keys_device", n=0, d_rec_keys=None, d_codes=None) == _lib.GF_OK


def test_no_cpu_fallback():
    """Host tensors (all there is without a GPU) are refused, and nothing is computed."""
    import numpy as np
    import torch
    from genefuserust_amd import Indexer
    from genefuserust_amd.fastq import FastqBatch
    ix = Indexer.from_gene_slices([b"ACGT" * 100])
    text = torch.from_numpy(np.frombuffer(b"@r:ACGT\nACGT\n+\nFFFF\n", dtype=np.uint8).copy())
    off = torch.tensor([0, 4], dtype=torch.int64)
    nl = torch.tensor([7, 12, 14, 19], dtype=torch.int64)
    batch = FastqBatch(text[8:12], text[15:19], off, 1, nl, 4, 0)
    keys = torch.ones(1, dtype=torch.int64)
    calls = (lambda: umi.cut_umis_device(ix, umi.Umi("read1", 2), batch),
             lambda: umi.name_umis_device(ix, text, batch),
             lambda: umi.mix_keys_device(ix, keys, torch.ones(1, dtype=torch.int64)))
    for call in calls:
        with pytest.raises(_lib.GfError) as e:
            call()
        assert e.value.code == _lib.GF_ERR_NO_DEVICE
    assert int(keys[0]) == 1
    with pytest.raises(ValueError, match="full FASTQ cut"):
        umi.cut_umis_device(ix, umi.Umi("read1", 2), batch._replace(qual_off=off))
    with pytest.raises(ValueError, match="inline source"):
        umi.cut_umis_device(ix, umi.Umi(), batch)
    with pytest.raises(ValueError, match="read2"):
        umi.cut_umis_device(ix, umi.Umi("read2", 2), batch)
