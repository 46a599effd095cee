"""CPU-side checks of libgfdeflate.so, the device deflate (include/gf_deflate.h): it loads next to libgfmatch.so, exports
what its header declares with the signatures deflate.py binds, is bound by INTEGRATION.md, its constants and capacity
functions are the header's and the bindings', it refuses bad arguments and short buffers before it touches a device, and
has no CPU fallback for the device call."""
import ctypes as C
import os
import re
import subprocess

import pytest

from genefuserust_amd import _lib, deflate
from tests import bgzf_members as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["gf_df_deflate_device", "gf_df_last_error", "gf_df_member_host", "gf_df_members", "gf_df_out_cap",
                "gf_df_workspace_bytes"]
PARAMETERS = {"gf_df_deflate_device": 10, "gf_df_last_error": 0, "gf_df_member_host": 5, "gf_df_members": 1,
              "gf_df_out_cap": 1, "gf_df_workspace_bytes": 1}


def _header() -> str:
    return open(os.path.join(ROOT, "include", "gf_deflate.h")).read()


def _declarations():
    """{entry point: [parameter type, ...]} of include/gf_deflate.h."""
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(gf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        out[name] = [] if params.strip() == "void" else [" ".join(p.split()[:-1]) for p in params.split(",")]
    return out


def test_header_declares_the_entry_points_and_states_the_format():
    d = _declarations()
    assert sorted(d) == ENTRY_POINTS and {k: len(v) for k, v in d.items()} == PARAMETERS
    flat = " ".join(_header().replace(" * ", " ").split())
    for phrase in ("members of GF_DF_TEXT_BYTES = 65280 bytes", "text of 0 bytes gives no member", "1f 8b 08 04 00000000 00 ff 0600",
                   "ONE final block", "dynamic Huffman codes", "stored when that is not longer", "31 bytes longer",
                   "every member fits 64 KiB", "end-of-file marker", "a function of the member's text alone",
                   "gf_df_core.h", "What may be READ", "up to 15 bytes", "ADDED into", "no CPU fallback",
                   "before anything is launched", "count as absent", "byte for byte"):
        assert phrase in flat, phrase
    kernels = open(os.path.join(ROOT, "genefuserust_amd", "scan_csrc", "gf_df_kernels.h")).read()
    core = open(os.path.join(ROOT, "genefuserust_amd", "scan_csrc", "gf_df_core.h")).read()
    assert '#include "gf_df_core.h"' in kernels and '#include "gf_if_core.h"' in core      # one encoder, the inflate's CRC
    assert "hip_runtime" not in core                                                      # the core is plain C++


def test_library_exports_and_signatures_match_the_header():
    L = deflate.lib()
    ctype_of = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    for name, params in _declarations().items():
        assert hasattr(L, name), "libgfdeflate.so does not export %s" % name
        want = [C.POINTER(C.c_int64) if p == "int64_t*" else C.c_void_p if "*" in p else ctype_of[p] for p in params]
        assert getattr(L, name).argtypes == want, name
    assert L.gf_df_last_error.restype == C.c_char_p and L.gf_df_deflate_device.restype == C.c_int
    for name in ("gf_df_members", "gf_df_out_cap", "gf_df_workspace_bytes"):
        assert getattr(L, name).restype == C.c_int64
    nm = subprocess.run(["nm", "-D", "--defined-only", deflate.DF_LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:   # nothing but the header's functions carries the library's prefix; the inflate's stay its own
        exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
        assert {s for s in exported if s.startswith("gf_df_")} == set(ENTRY_POINTS)
        assert not {s for s in exported if s.startswith(("gf_if_", "gf_rw_"))}


def test_library_needs_libgfmatch_next_to_it():
    out = subprocess.run(["readelf", "-d", deflate.DF_LIB_PATH], capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("readelf not available")
    assert "[libgfmatch.so]" in out.stdout and "$ORIGIN" in out.stdout
    assert "libgfinflate" not in out.stdout and "libgfwrite" not in out.stdout


def test_makefile_builds_the_library_with_the_others():
    mk = open(os.path.join(ROOT, "genefuserust_amd", "scan_csrc", "Makefile")).read()
    for target in ("all:", "resource-usage:", "\trm -f"):
        line = next(x for x in mk.splitlines() if x.startswith(target))
        assert "gfdeflate" in line or "gf_deflate.hip" in line, target
    assert "../libgfdeflate.so: gf_deflate.hip $(HDRS) ../libgfmatch.so" in mk
    assert "-c -o /dev/null gf_deflate.hip" in mk and "libgfdeflate.so" in mk.split("HIPCC ?=")[0]
    assert "libgfdeflate.so" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_integration_doc_binds_every_entry_point():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = doc.index('extern "C" {', doc.index("src/gfdeflate_sys.rs"))
    block = doc[start:doc.index("\n}", start)]
    assert sorted(set(re.findall(r"pub fn (gf_[a-z0-9_]+)\(", block))) == ENTRY_POINTS
    for name, params in _declarations().items():
        bound = re.search(r"pub fn %s\(([^)]*)\)" % name, block).group(1)
        assert len([p for p in bound.split(",") if p.strip()]) == len(params), name
    section = doc[doc.index("src/gfdeflate_sys.rs"):start]
    assert "pub const GF_DF_TEXT_BYTES: i64 = 65280;" in section and "pub const GF_DF_TOTALS: usize = 5;" in section


def test_constants_and_capacities_are_the_headers():
    h = _header()
    assert "#define GF_DF_TEXT_BYTES 65280" in h and "#define GF_DF_STORED_BYTES_OVER 31" in h
    assert "#define GF_DF_TOTALS 5" in h and "#define GF_DF_EOF_MARKER_BYTES 28" in h
    assert (deflate.TEXT, deflate.STORED_OVER, deflate.TOTALS) == (65280, 31, 5)
    assert deflate.EOF_MARKER == bm.EOF_MARKER and len(deflate.EOF_MARKER) == 28
    marker = re.search(r'#define GF_DF_EOF_MARKER "([^"]*)"', h).group(1)
    assert marker.encode().decode("unicode_escape").encode("latin-1") == deflate.EOF_MARKER
    L = deflate.lib()
    caps = (-5, 0, 1, 2, 65279, 65280, 65281, 2 * 65280, 2 * 65280 + 1, 1 << 26, (1 << 32) + 7, 1 << 40)
    for cap in caps:
        members = 0 if cap <= 0 else -(-cap // 65280)
        assert L.gf_df_members(cap) == members == deflate.members(cap), cap
        assert L.gf_df_out_cap(cap) == max(cap, 0) + 31 * members == deflate.out_cap(cap), cap
    for fn in (L.gf_df_members, L.gf_df_out_cap, L.gf_df_workspace_bytes):
        sizes = [fn(cap) for cap in caps]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0]                # non-decreasing
    # per member a 64 KiB slot and 2 * 65280 bytes of tokens; the sizes in 256-byte pieces, and 256 bytes to align
    assert L.gf_df_workspace_bytes(65280) == 65536 + 2 * 65280 + 256 + 256
    assert L.gf_df_workspace_bytes(65281) - L.gf_df_workspace_bytes(65280) == 65536 + 2 * 65280
    assert L.gf_df_workspace_bytes(0) >= 0


CAP = 100000


def _call(text=True, length=False, out=True, out_cap=None, off=True, totals=True, workspace=True, workspace_bytes=None,
          cap=CAP):
    """The call over host memory that is never dereferenced: the checks come first."""
    L = deflate.lib()
    buf = (C.c_char * 256)()
    dummy = C.cast(buf, C.c_void_p)
    return L.gf_df_deflate_device(dummy if text else None, cap, dummy if length else None, dummy if out else None,
                                  L.gf_df_out_cap(cap) if out_cap is None else out_cap, dummy if off else None,
                                  dummy if totals else None, dummy if workspace else None,
                                  L.gf_df_workspace_bytes(cap) if workspace_bytes is None else workspace_bytes, None)


def test_argument_errors_without_a_device():
    ARG, NODEV, CAPACITY = _lib.GF_ERR_ARG, _lib.GF_ERR_NO_DEVICE, _lib.GF_ERR_CAPACITY
    L = deflate.lib()
    err = L.gf_df_last_error
    assert _call() == NODEV and b"no CPU fallback" in err()          # host memory
    assert _call(length=True) == NODEV
    assert _call(cap=-1) == ARG and b"negative" in err()
    assert _call(cap=(1 << 40) + 1) == ARG and b"out of range" in err()
    assert _call(off=False) == ARG and b"member offsets or totals" in err()
    assert _call(totals=False) == ARG and b"member offsets or totals" in err()
    assert _call(text=False) == ARG and b"null text or output" in err()
    assert _call(out=False) == ARG and b"null text or output" in err()
    assert _call(out_cap=-1) == ARG and _call(workspace_bytes=-1) == ARG and b"negative" in err()
    # an output, a workspace one byte short: refused before anything is launched
    assert _call(out_cap=L.gf_df_out_cap(CAP) - 1) == CAPACITY and b"gf_df_out_cap" in err()
    assert _call(workspace_bytes=L.gf_df_workspace_bytes(CAP) - 1) == CAPACITY and b"gf_df_workspace_bytes" in err()
    assert _call(workspace=False) == CAPACITY
    # no text at all needs neither text nor output nor workspace
    assert _call(cap=0, text=False, out=False, workspace=False, workspace_bytes=0, out_cap=0) == NODEV


def test_member_host_refusals():
    ARG, CAPACITY = _lib.GF_ERR_ARG, _lib.GF_ERR_CAPACITY
    L = deflate.lib()
    out = C.create_string_buffer(70000)
    size = C.c_int64(-1)
    text = bm.fastq_text(3000)
    assert L.gf_df_member_host(text, 0, out, 70000, C.byref(size)) == ARG and b"1 .. 65280" in L.gf_df_last_error()
    assert L.gf_df_member_host(text, 65281, out, 70000, C.byref(size)) == ARG
    assert L.gf_df_member_host(None, 10, out, 70000, C.byref(size)) == ARG and b"null" in L.gf_df_last_error()
    assert L.gf_df_member_host(text, 3000, None, 70000, C.byref(size)) == ARG
    assert L.gf_df_member_host(text, 3000, out, 70000, None) == ARG
    assert L.gf_df_member_host(text, 3000, out, 70000, C.byref(size)) == 0 and 26 < size.value < 3000
    member = out.raw[:size.value]
    assert L.gf_df_member_host(text, 3000, out, size.value - 1, C.byref(size)) == CAPACITY
    assert L.gf_df_member_host(text, 3000, out, size.value, C.byref(size)) == 0 and out.raw[:size.value] == member
    assert deflate.deflate_member_host(text) == member and deflate.deflate_host(text * 30)[:len(member)] != b""
    for bad in (b"", b"x" * 65281):
        with pytest.raises(ValueError, match="1 .. 65280"):
            deflate.deflate_member_host(bad)


def test_no_cpu_fallback():
    """Host tensors (all there is without a GPU) are refused, and nothing is computed."""
    import numpy as np
    import torch
    text = torch.from_numpy(np.frombuffer(bm.fastq_text(1000), dtype=np.uint8).copy())
    with pytest.raises(_lib.GfError) as e:
        deflate.deflate_device(text)
    assert e.value.code == _lib.GF_ERR_NO_DEVICE
