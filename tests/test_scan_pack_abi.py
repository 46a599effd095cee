"""CPU-side checks of libgfpack.so, the outputs of K scans packed into one block (include/gf_scan_pack.h): it loads next
to libgfmatch.so, exports what its header declares, is bound by INTEGRATION.md, sizes its block sensibly, rejects bad
arguments before it touches a device, and has no CPU fallback.  Plus the block's layout without a device:
``scan_pack.unpack_block`` takes apart what ``tests/pack_model.py`` puts together."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.pack_model import (BAD_SCAN, OVER_HITS, OVER_NAMES, OVER_RETRY, make_scan, pack_model, piece_kinds, plan,
                              same_scans)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "genefuserust_amd", "scan_csrc", "gf_pk_kernels.h")
ENTRY_POINTS = ["gf_pk_block_bytes", "gf_pk_last_error", "gf_pk_pack_device", "gf_pk_workspace_bytes"]


def source_define(name: str) -> int:
    """An integer ``#define`` of gf_pk_kernels.h, read from the source."""
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, open(KERNELS).read(), flags=re.M)
    assert m, name
    return int(m.group(1))


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "gf_scan_pack.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gf_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_entry_points():
    assert _declared_functions() == ENTRY_POINTS


def test_library_exports_every_declared_symbol():
    from genefuserust_amd import scan_pack
    L = scan_pack.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), "libgfpack.so does not export %s" % name


def test_library_needs_libgfmatch_next_to_it():
    out = subprocess.run(["readelf", "-d", os.path.join(ROOT, "genefuserust_amd", "libgfpack.so")],
                         capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("readelf not available")
    assert "[libgfmatch.so]" in out.stdout and "$ORIGIN" in out.stdout


def test_integration_doc_binds_every_entry_point():
    """INTEGRATION.md's fifth `extern "C"` block (after the one of gf_hit_names.h) binds every function of
    gf_scan_pack.h, and its struct has the fields of gf_pk_scan in the header's order."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = doc.index('extern "C" {', doc.index("pub fn gf_hn_last_error()"))
    block = doc[start:doc.index("}", start)]
    bound = sorted(set(re.findall(r"pub fn (gf_[a-z0-9_]+)\(", block)))
    assert bound == ENTRY_POINTS
    header = open(os.path.join(ROOT, "include", "gf_scan_pack.h")).read()
    struct = header[header.index("typedef struct gf_pk_scan {"):header.index("} gf_pk_scan;")]
    fields = re.findall(r"\b(d_[a-z_]+|[a-z]+_cap)\b(?=[;,])", re.sub(r"/\*.*?\*/", "", struct, flags=re.S))
    rust = doc[doc.index("pub struct gf_pk_scan {"):start]
    assert re.findall(r"pub ([a-z_]+):", rust) == fields and len(fields) == 10


def test_descriptor_dtype_is_the_headers_struct():
    """scan_pack.SCAN_DTYPE against the struct as a C compiler lays it out: ten 8-byte fields in the header's order."""
    from genefuserust_amd import scan_pack
    header = open(os.path.join(ROOT, "include", "gf_scan_pack.h")).read()
    struct = header[header.index("typedef struct gf_pk_scan {"):header.index("} gf_pk_scan;")]
    fields = re.findall(r"\b(d_[a-z_]+|[a-z]+_cap)\b(?=[;,])", re.sub(r"/\*.*?\*/", "", struct, flags=re.S))
    assert [("d_" + n) if not n.endswith("_cap") else n for n in scan_pack.SCAN_DTYPE.names] == fields
    assert scan_pack.SCAN_DTYPE.itemsize == 80
    assert [scan_pack.SCAN_DTYPE.fields[n][1] for n in scan_pack.SCAN_DTYPE.names] == list(range(0, 80, 8))


def test_block_bytes_is_monotone_and_exact():
    from genefuserust_amd import scan_pack
    L = scan_pack.lib()
    vals = [0, 1, 2, 15, 16, 17, 1024, 4097, 1 << 20]
    for fixed in vals[:4]:
        for pos in range(4):
            sizes = []
            for v in vals:
                args = [fixed] * 4
                args[pos] = v
                sizes.append(L.gf_pk_block_bytes(*args))
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), (pos, fixed, sizes)
    for pos in range(4):
        args = [3, 3, 3, 3]
        args[pos] = -1
        assert L.gf_pk_block_bytes(*args) == 0
    assert L.gf_pk_block_bytes(1, 0, 0, 0) == 64 * 2 + 16      # the headers and one name offset, padded
    assert L.gf_pk_workspace_bytes(-1) == 0
    ws = [L.gf_pk_workspace_bytes(k) for k in (1, 2, 64, 65, 1024)]
    assert all(a <= b for a, b in zip(ws, ws[1:])) and ws[0] >= 8 * 11
    # with the true sums it is the model's block, to the byte
    rng = np.random.default_rng(3)
    scans = [make_scan(rng, r, b, n) for r, b, n in ((0, 0, 0), (1, 15, 1), (2, 17, 16), (300, 4097, 4097))]
    rows, _ = plan(scans)
    assert L.gf_pk_block_bytes(4, int(rows[:, 0].sum()), int(rows[:, 1].sum()), int(rows[:, 2].sum())) \
        == len(pack_model(scans))


def _pack(L, k=2, scans=True, ws=True, ws_bytes=1 << 20, block=True, block_bytes=1 << 20, misalign=0):
    buf = (C.c_char * 512)()
    base = C.addressof(buf)
    base += -base % 16
    dummy = C.c_void_p(base)
    return L.gf_pk_pack_device(dummy if scans else None, k, dummy if ws else None, ws_bytes,
                               C.c_void_p(base + misalign) if block else None, block_bytes, None)


def test_argument_errors_without_a_device():
    from genefuserust_amd import _lib, scan_pack
    L = scan_pack.lib()
    for k in (0, 1025, -1):
        assert _pack(L, k=k) == _lib.GF_ERR_ARG, k
        assert b"number of scans" in L.gf_pk_last_error()
    assert _pack(L, scans=False) == _lib.GF_ERR_ARG
    assert b"null scans" in L.gf_pk_last_error()
    assert _pack(L, block=False) == _lib.GF_ERR_ARG
    assert b"null block" in L.gf_pk_last_error()
    assert _pack(L, ws=False) == _lib.GF_ERR_ARG
    for neg in (dict(block_bytes=-1), dict(ws_bytes=-5)):
        assert _pack(L, **neg) == _lib.GF_ERR_ARG, neg
        assert b"negative" in L.gf_pk_last_error()
    assert _pack(L, misalign=8) == _lib.GF_ERR_ARG
    assert b"aligned" in L.gf_pk_last_error()
    assert _pack(L, ws_bytes=8) == _lib.GF_ERR_CAPACITY
    assert b"gf_pk_workspace_bytes" in L.gf_pk_last_error()
    assert _pack(L, k=2, block_bytes=64 * 3 - 1) == _lib.GF_ERR_CAPACITY     # not even the headers
    assert b"headers" in L.gf_pk_last_error()
    assert _pack(L) == _lib.GF_ERR_NO_DEVICE                                 # host memory: there is no CPU fallback
    assert b"not device memory" in L.gf_pk_last_error()


def test_pack_scans_device_raises_without_a_device():
    """No CPU fallback: host tensors (all there is without a GPU) are refused, and so is a K out of range."""
    import torch
    from genefuserust_amd import _lib
    from genefuserust_amd.hit_names import HitNames
    from genefuserust_amd.read_pair import PairScan
    from genefuserust_amd.scan_pack import pack_scans_device
    u8 = torch.zeros(64, dtype=torch.uint8)
    scan = PairScan(torch.zeros((4, 64), dtype=torch.uint8), u8, u8, torch.zeros(8, dtype=torch.int64))
    names = HitNames(u8, torch.zeros(5, dtype=torch.int64), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(_lib.GfError) as e:
        pack_scans_device([scan], [names])
    assert e.value.code == _lib.GF_ERR_NO_DEVICE
    for scans, nm in (([], []), ([scan] * 1025, [names] * 1025), ([scan, scan], [names])):
        with pytest.raises(_lib.GfError) as e:
            pack_scans_device(scans, nm)
        assert e.value.code == _lib.GF_ERR_ARG


def _hand_built(rng):
    """Clean scans, one with zero records, and one of each kind that is packed as empty, between clean ones."""
    return [make_scan(rng, 2, 33, 20, missing=1), make_scan(rng, 0, 0, 0), make_scan(rng, 5, 160, 7),
            make_scan(rng, 4, 50, 9, over=OVER_RETRY), make_scan(rng, 1, 1, 1),
            make_scan(rng, 4, 50, 9, over=OVER_HITS), make_scan(rng, 3, 16, 16),
            make_scan(rng, 4, 50, 9, names_over=True), make_scan(rng, 300, 4097, 4097)]


def test_unpack_block_inverts_the_model():
    from genefuserust_amd.scan_pack import unpack_block
    scans = _hand_built(np.random.default_rng(11))
    block = pack_model(scans)
    got = unpack_block(block, len(scans))
    same_scans(got, scans)
    assert [u.bits for u in got] == [0, 0, 0, OVER_RETRY, 0, OVER_HITS, 0, OVER_NAMES, 0]
    assert [len(u.rec) for u in got] == [2, 0, 5, 0, 1, 0, 3, 0, 300] and got[0].missing == 1
    # the overflowed ones: empty, the true counts in the header
    assert got[5].totals["hits"] == int(scans[5].totals[0]) > scans[5].hits.shape[0] and got[5].names == []
    assert got[7].name_bytes == int(scans[7].name_totals[1]) > scans[7].names.size
    assert got[3].totals["retried_reads"] == 7 and got[3].bases == b""
    # a record's seq_offset and its names are its own scan's
    assert got[8].names == [scans[8].names[scans[8].name_off[j]:scans[8].name_off[j + 1]].tobytes() for j in range(300)]
    # the padding is zero and every section starts on the grid: the block's size is the size function's (see above);
    # a trailing byte more or less is refused
    from_unpadded = unpack_block(block + b"\0" * 5, len(scans))
    same_scans(from_unpadded, scans)
    for bad in (block[:-1], block[:64], pack_model(scans, block_bytes=len(block) - 1)):
        with pytest.raises(ValueError):
            unpack_block(bad, len(scans))
    with pytest.raises(ValueError):
        unpack_block(block, len(scans) - 1)


def test_model_refuses_what_does_not_hold_together():
    """A count beyond its capacity without the scan's own bit, names of another number of records, a first offset
    outside the names: BAD_SCAN, packed as empty."""
    rng = np.random.default_rng(5)
    a, b, c = make_scan(rng, 3, 30, 10), make_scan(rng, 3, 30, 10), make_scan(rng, 3, 30, 10)
    a.totals[0] = a.hits.shape[0] + 1
    b.name_totals[0] = 2
    c.name_off[0] = c.names.size
    rows, parts = plan([a, make_scan(rng, 1, 5, 3), b, c])
    assert [int(r[7]) & 255 for r in rows] == [BAD_SCAN, 0, BAD_SCAN, BAD_SCAN]
    assert all(p.size == 0 for k in (0, 2, 3) for p in parts[k]) and rows[1, 0] == 1


def test_piece_kinds_of_the_device_cases_all_occur():
    """The sources of tests/test_scan_pack.py's K >= 16 cases, scan k sliced k mod 16 bytes off the grid: pieces copied
    whole from a co-aligned source, pieces put together bytewise and pieces across two parts all occur."""
    rng = np.random.default_rng(2)
    scans = [make_scan(rng, k % 4, (0, 1, 15, 16, 17, 4097)[k % 6], (0, 1, 15, 16, 17, 4097)[(k + 1) % 6] if k % 4 else 0)
             for k in range(64)]
    kinds = piece_kinds(scans, [{s: k % 16 for s in ("records", "bases", "quals", "names")} for k in range(64)])
    assert all(kinds[x] > 0 for x in ("aligned", "bytewise", "straddle", "offsets")), kinds
    assert sum(kinds.values()) * 16 == len(pack_model(scans)) - 64 * 65


def test_copy_grid_constants():
    """The copy kernel's piece is the block's grid, and one pass of its capped grid is what the device test steps
    past."""
    assert source_define("GF_PK_PIECE") == 16
    assert source_define("GF_PK_COPY_BLOCKS") >= 1 and source_define("GF_PK_SECTIONS") == 5
    header = open(os.path.join(ROOT, "include", "gf_scan_pack.h")).read()
    assert int(re.search(r"#define GF_PK_MAX_SCANS (\d+)", header).group(1)) == 1024
