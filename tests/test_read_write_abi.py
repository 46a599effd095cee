"""CPU-side checks of libgfwrite.so, the FASTQ output (include/gf_read_write.h): it loads next to libgfmatch.so, exports
what its header declares with the signatures read_write.py binds, is bound by INTEGRATION.md, its constants are the
bindings', it refuses bad settings and arguments before it touches a device, and has no CPU fallback."""
import ctypes as C
import os
import re
import subprocess

import pytest

from genefuserust_amd import _lib, read_write
from tests import read_write_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["gf_rw_format_device", "gf_rw_last_error", "gf_rw_workspace_bytes"]
PARAMETERS = {"gf_rw_format_device": 9, "gf_rw_workspace_bytes": 1, "gf_rw_last_error": 0}
SIDE_FIELDS = ["d_text", "text_bytes", "d_nl_pos", "newlines", "d_bases", "d_quals", "d_off", "d_pre_bases", "d_pre_off",
               "d_out_text", "out_cap", "d_out_off"]


def _header() -> str:
    return open(os.path.join(ROOT, "include", "gf_read_write.h")).read()


def _declarations():
    """{entry point: [parameter type, ...]} of include/gf_read_write.h."""
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(gf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        out[name] = [] if params.strip() == "void" else [" ".join(p.split()[:-1]) for p in params.split(",")]
    return out


def _struct_fields(name: str):
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
    return [(f.split()[-1].lstrip("*"), "*" in f) for f in body.split(";") if f.strip()]


def test_header_declares_the_entry_points_and_states_the_predicate():
    d = _declarations()
    assert sorted(d) == ENTRY_POINTS and {k: len(v) for k, v in d.items()} == PARAMETERS
    flat = " ".join(_header().replace(" * ", " ").split())
    for phrase in ("When a record is written", "its mate's is too", "keep file order", "R1 and R2 stay in step",
                   "The four lines", "line 4 i of that side's text", "byte 0 for i = 0", "The bytes are verbatim",
                   "before the first space or tab", "umi1 + '_' + umi2", "Both mates of a pair get the same tag",
                   "the case of the bytes is kept", "input record + 1 + the tag", "no overflow retry", "ADDED into",
                   "no CPU fallback", "up to 15 bytes", "Offsets are 64-bit", "No byte outside a record's own output span"):
        assert phrase in flat, phrase
    core = open(os.path.join(ROOT, "genefuserust_amd", "scan_csrc", "gf_rw_core.h")).read()
    assert '#include "gf_um_core.h"' in core       # the name line and the sources are the UMI calls', not a copy
    kernels = open(os.path.join(ROOT, "genefuserust_amd", "scan_csrc", "gf_rw_kernels.h")).read()
    host = open(os.path.join(ROOT, "genefuserust_amd", "scan_csrc", "gf_read_write.hip")).read()
    assert '#include "gf_pp_kernels.h"' in kernels and "gf_pp_k_scan<2>" in host      # the read filter's offsets scan, as it is


def test_library_exports_and_signatures_match_the_header():
    L = read_write.lib()
    ctype_of = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    for name, params in _declarations().items():
        assert hasattr(L, name), "libgfwrite.so does not export %s" % name
        assert getattr(L, name).argtypes == [C.c_void_p if "*" in p else ctype_of[p] for p in params], name
    assert L.gf_rw_last_error.restype == C.c_char_p and L.gf_rw_workspace_bytes.restype == C.c_int64
    assert L.gf_rw_format_device.restype == C.c_int
    nm = subprocess.run(["nm", "-D", "--defined-only", read_write.RW_LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:   # nothing but the header's functions carries the library's prefix
        exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
        assert {s for s in exported if s.startswith("gf_rw_")} == set(ENTRY_POINTS)
        assert not {s for s in exported if s.startswith(("gf_um_", "gf_pp_", "gf_dd_"))}   # the others' calls stay theirs


def test_the_structs_are_the_bindings():
    side = _struct_fields("gf_rw_side")
    assert [n for n, _ in side] == SIDE_FIELDS == [n for n, _ in read_write.GfRwSide._fields_]
    for (name, pointer), (_, ctype) in zip(side, read_write.GfRwSide._fields_):
        assert ctype is (C.c_void_p if pointer else C.c_int64), name
    assert C.sizeof(read_write.GfRwSide) == 12 * 8
    settings = _struct_fields("gf_rw_settings")
    assert [n for n, _ in settings] == ["umi_source", "umi_length", "gather"] == \
        [n for n, _ in read_write.GfRwSettings._fields_]
    assert C.sizeof(read_write.GfRwSettings) == 12


def test_library_needs_libgfmatch_next_to_it():
    out = subprocess.run(["readelf", "-d", read_write.RW_LIB_PATH], capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("readelf not available")
    assert "[libgfmatch.so]" in out.stdout and "$ORIGIN" in out.stdout
    assert "libgfumi" not in out.stdout and "libgfprep" not in out.stdout


def test_makefile_builds_the_library_with_the_others():
    mk = open(os.path.join(ROOT, "genefuserust_amd", "scan_csrc", "Makefile")).read()
    for target in ("all:", "resource-usage:", "\trm -f"):
        line = next(x for x in mk.splitlines() if x.startswith(target))
        assert "gfwrite" in line or "gf_read_write.hip" in line, target
    assert "../libgfwrite.so: gf_read_write.hip $(HDRS) ../libgfmatch.so" in mk
    assert "-c -o /dev/null gf_read_write.hip" in mk and "libgfwrite.so" in mk.split("HIPCC ?=")[0]
    assert "libgfwrite.so" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_integration_doc_binds_every_entry_point():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = doc.index('extern "C" {', doc.index("src/gfwrite_sys.rs"))
    block = doc[start:doc.index("\n}", start)]
    assert sorted(set(re.findall(r"pub fn (gf_[a-z0-9_]+)\(", block))) == ENTRY_POINTS
    for name, params in _declarations().items():
        bound = re.search(r"pub fn %s\(([^)]*)\)" % name, block).group(1)
        assert len([p for p in bound.split(",") if p.strip()]) == len(params), name
    section = doc[doc.index("src/gfwrite_sys.rs"):start]
    struct = re.search(r"pub struct gf_rw_side \{(.*?)\n\}", section, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", struct) == SIDE_FIELDS
    assert "pub const GF_RW_TOTALS: usize = 5;" in section and "GF_RW_TAG_MAX: i64 = 1 + 32 + 1 + 32;" in section


def test_constants_are_the_bindings_and_the_models():
    h = _header()
    assert "#define GF_RW_TAG_MAX (1 + 32 + 1 + 32)" in h and "#define GF_RW_TOTALS 5" in h
    assert read_write.TAG_MAX == model.TAG_MAX == 66 and read_write.TOTALS == model.TOTALS == 5
    assert (read_write.WIDE, read_write.BYTES) == (model.WIDE, model.BYTES) == (0, 1)
    assert "#define GF_RW_WIDE 0" in h and "#define GF_RW_BYTES 1" in h
    for text_bytes, n in ((0, 0), (1, 1), (1000, 7), (1 << 33, 1 << 27)):
        assert read_write.capacity(text_bytes, n) == model.capacity(text_bytes, n) == text_bytes + 1 + 66 * n
    assert read_write.lib().gf_rw_workspace_bytes(-1) == 0
    sizes = [read_write.lib().gf_rw_workspace_bytes(n) for n in (0, 1, 255, 256, 257, 600, 1 << 20, 1 << 30)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] > sizes[0]


N = 10
TEXT_BYTES = 100


def _side(**over):
    buf = (C.c_char * 256)()
    dummy = C.cast(buf, C.c_void_p).value
    values = {name: dummy if ctype is C.c_void_p else 0 for name, ctype in read_write.GfRwSide._fields_}
    values.update(text_bytes=TEXT_BYTES, newlines=40, out_cap=model.capacity(TEXT_BYTES, N))
    values.update(over)
    side = read_write.GfRwSide(**values)
    side._keep = buf
    return side


def _call(idx=True, settings=(0, 0, 0), left=None, right=None, single=False, n=N, workspace=True,
          workspace_bytes=1 << 20, totals=True):
    """The call over host memory that is never dereferenced: the checks come first."""
    L = read_write.lib()
    buf = (C.c_char * 256)()
    dummy = C.cast(buf, C.c_void_p)
    config = None if settings is None else read_write.GfRwSettings(*settings)
    left = _side() if left is None else left
    right = None if single else (_side() if right is None else right)
    return L.gf_rw_format_device(dummy if idx else None, None if config is None else C.addressof(config),
                                 None if left is False else C.addressof(left),
                                 None if right is None else C.addressof(right), n, dummy if workspace else None,
                                 workspace_bytes, dummy if totals else None, None)


def test_every_refused_setting_gives_an_argument_error_with_a_message():
    ARG, NODEV = _lib.GF_ERR_ARG, _lib.GF_ERR_NO_DEVICE
    err = read_write.lib().gf_rw_last_error
    refused = 0
    for source in (-1, 0, 1, 2, 3, 4, 99):
        for length in (-1, 0, 1, 8, 32, 33):
            for gather in (-1, 0, 1, 2):
                rc = _call(settings=(source, length, gather))
                if model.settings_ok(source, length, gather):
                    assert rc == NODEV, (source, length, gather)       # accepted: the next check is the memory's
                else:
                    refused += 1
                    assert rc == ARG and b"settings out of range" in err(), (source, length, gather)
    assert refused == 7 * 6 * 4 - 2 * (1 + 3 * 3)
    # read2 with single-end input
    assert _call(settings=(2, 8, 0), single=True) == ARG and b"read2" in err()
    assert _call(settings=(1, 8, 0), single=True) == NODEV
    assert _call(settings=(3, 8, 0), single=True) == NODEV      # per_read is read1 there
    assert _call(settings=None) == ARG and b"settings" in err()


def test_argument_errors_without_a_device():
    ARG, NODEV, CAP = _lib.GF_ERR_ARG, _lib.GF_ERR_NO_DEVICE, _lib.GF_ERR_CAPACITY
    err = read_write.lib().gf_rw_last_error
    assert _call(idx=False) == ARG and b"null index" in err()
    assert _call(totals=False) == ARG and b"totals" in err()
    assert _call(left=False) == ARG and b"null side" in err()
    assert _call() == NODEV and b"no CPU fallback" in err()      # host memory
    assert _call(single=True) == NODEV
    assert _call(n=-1) == ARG and b"negative" in err()
    assert _call(n=(1 << 38) + 1) == ARG and b"out of range" in err()
    for where in ("left", "right"):
        for hole, word in (("d_text", b"text"), ("d_nl_pos", b"newline"), ("d_off", b"offsets"), ("d_out_off", b"offsets"),
                           ("d_bases", b"bases or qualities"), ("d_quals", b"bases or qualities"),
                           ("d_out_text", b"output text")):
            assert _call(**{where: _side(**{hole: None})}) == ARG and word in err(), (where, hole)
        for size in ("text_bytes", "newlines", "out_cap"):
            assert _call(**{where: _side(**{size: -1})}) == ARG and b"negative" in err(), (where, size)
        # an output one byte short of the capacity
        assert _call(**{where: _side(out_cap=model.capacity(TEXT_BYTES, N) - 1)}) == CAP and b"GF_RW_CAPACITY" in err()
        assert _call(**{where: _side(out_cap=model.capacity(TEXT_BYTES, N))}) == NODEV
        # no tag: the pre-cut batches may be NULL; with one they may not
        bare = dict(d_pre_bases=None, d_pre_off=None)
        assert _call(**{where: _side(**bare)}) == NODEV
        assert _call(settings=(3, 8, 0), **{where: _side(**bare)}) == ARG and b"pre-cut" in err()
        assert _call(settings=(1, 8, 0), **{where: _side(d_pre_off=None)}) == ARG and b"pre-cut" in err()
        # an empty text needs no pointers to it
        assert _call(**{where: _side(d_text=None, text_bytes=0, d_nl_pos=None, newlines=0,
                                     out_cap=model.capacity(0, N))}) == NODEV
    # a workspace one byte short
    need = read_write.lib().gf_rw_workspace_bytes(N)
    assert _call(workspace_bytes=-1) == ARG and b"negative" in err()
    assert _call(workspace_bytes=need - 1) == CAP and b"gf_rw_workspace_bytes" in err()
    assert _call(workspace_bytes=need) == NODEV
    assert _call(workspace=False) == CAP
    # no records: the bases, the qualities and the workspace may be NULL, the capacity is text_bytes + 1
    empty = dict(d_bases=None, d_quals=None, out_cap=TEXT_BYTES + 1)
    assert _call(n=0, left=_side(**empty), right=_side(**empty), workspace=False, workspace_bytes=0) == NODEV
    assert _call(n=0, left=_side(**dict(empty, out_cap=TEXT_BYTES))) == CAP


def test_no_cpu_fallback():
    """Host tensors (all there is without a GPU) are refused, and nothing is computed."""
    import numpy as np
    import torch
    from genefuserust_amd import Indexer
    from genefuserust_amd.fastq import FastqBatch
    from genefuserust_amd.umi import Umi
    ix = Indexer.from_gene_slices([b"ACGT" * 100])
    text = torch.from_numpy(np.frombuffer(b"@r:ACGT\nACGT\n+\nFFFF\n", dtype=np.uint8).copy())
    off = torch.tensor([0, 4], dtype=torch.int64)
    nl = torch.tensor([7, 12, 14, 19], dtype=torch.int64)
    batch = FastqBatch(text[8:12], text[15:19], off, 1, nl, 4, 0)
    with pytest.raises(_lib.GfError) as e:
        read_write.format_reads_device(ix, [text], [batch], [batch], 1)
    assert e.value.code == _lib.GF_ERR_NO_DEVICE
    with pytest.raises(ValueError, match="full FASTQ cut"):
        read_write.format_reads_device(ix, [text], [batch], [batch._replace(qual_off=off)], 1)
    with pytest.raises(ValueError, match="together"):
        read_write.format_reads_device(ix, [text], [batch], [batch], 1, umi=Umi("read1", 2))
    with pytest.raises(ValueError, match="inline"):
        read_write.format_reads_device(ix, [text], [batch], [batch], 1, pre=[batch], umi=Umi())
    with pytest.raises(ValueError, match="read2"):
        read_write.format_reads_device(ix, [text], [batch], [batch], 1, pre=[batch], umi=Umi("read2", 2))
