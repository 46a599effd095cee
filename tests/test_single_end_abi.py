"""CPU-side checks of libgfse.so, the single-end scan (include/gf_single_end.h): it loads next to libgfmatch.so,
exports what its header declares, is bound by INTEGRATION.md, sizes its workspace sensibly, rejects bad arguments
before it touches a device, and has no CPU fallback."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "gf_single_end.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gf_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_entry_points():
    assert _declared_functions() == ["gf_se_last_error", "gf_se_retry_capacity", "gf_se_scan_device",
                                     "gf_se_workspace_bytes"]


def test_library_exports_every_declared_symbol():
    from genefuserust_amd import single_end
    L = single_end.lib()
    for name in _declared_functions():
        assert hasattr(L, name), "libgfse.so does not export %s" % name


def test_library_needs_libgfmatch_next_to_it():
    out = subprocess.run(["readelf", "-d", os.path.join(ROOT, "genefuserust_amd", "libgfse.so")], capture_output=True,
                         text=True)
    if out.returncode != 0:
        pytest.skip("readelf not available")
    assert "[libgfmatch.so]" in out.stdout and "$ORIGIN" in out.stdout


def test_integration_doc_binds_every_entry_point():
    """INTEGRATION.md's second `extern "C"` block (after the one of gfmatch.h) binds every function of
    gf_single_end.h."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    first = doc.index('extern "C" {')
    start = doc.index('extern "C" {', doc.index("pub fn last_error()", first))
    block = doc[start:doc.index("}", start)]
    bound = set(re.findall(r"pub fn (gf_[a-z0-9_]+)\(", block))
    missing = [n for n in _declared_functions() if n not in bound]
    assert not missing, missing


def test_workspace_is_monotone_and_retry_capacity_has_a_floor():
    from genefuserust_amd import single_end
    L = single_end.lib()
    ns = [0, 1, 100, 4095, 4096, 4097, 65536, 1 << 20, 20_000_000]
    for L_ in (1, 150, 300, 4096):
        for rc in (0, 1, 17, 4096, 1 << 20):
            w = [L.gf_se_workspace_bytes(n, L_, rc) for n in ns]
            assert all(a <= b for a, b in zip(w, w[1:])), (L_, rc, w)
        for n in ns:
            w = [L.gf_se_workspace_bytes(n, L_, rc) for rc in (1, 2, 100, 4096, 1 << 20, 1 << 30)]
            assert all(a <= b for a, b in zip(w, w[1:])), (L_, n, w)
    # the default retry slots are part of the size: a larger default never shrinks the workspace
    assert L.gf_se_workspace_bytes(1 << 20, 150, 0) >= L.gf_se_workspace_bytes(1 << 20, 150, 1)
    # a first pass per read (count, status, two matches) at the very least
    assert L.gf_se_workspace_bytes(1 << 20, 150, 1) >= (1 << 20) * 34
    for n in (0, 1, 1000, 4096, 100_000, 20_000_000):
        assert L.gf_se_retry_capacity(n) >= 4096
    assert L.gf_se_retry_capacity(20_000_000) >= 20_000_000 // 64
    assert L.gf_se_workspace_bytes(-1, 150, 0) == 0 and L.gf_se_workspace_bytes(10, -1, 0) == 0


def _scan(L, idx=None, n=10, max_len=150, n_bytes=1500, hits_cap=0, bytes_cap=0, totals=True, ws_bytes=1 << 20,
          hits=None, hb=None, n_genes=0):
    buf = (C.c_char * 64)()
    t = C.cast(buf, C.c_void_p) if totals else None
    dummy = C.cast(buf, C.c_void_p)
    return L.gf_se_scan_device(idx, dummy, dummy, dummy, n_bytes, n, max_len, None, n_genes, 0, 0, dummy, ws_bytes,
                               hits, hits_cap, hb, hb, bytes_cap, t, None)


def test_argument_errors_without_a_device():
    from genefuserust_amd import _lib, single_end
    L = single_end.lib()
    assert _scan(L) == _lib.GF_ERR_ARG                                   # null index
    assert b"null index" in L.gf_se_last_error()
    assert _scan(L, totals=False) == _lib.GF_ERR_ARG
    assert _scan(L, n=-1) == _lib.GF_ERR_ARG                             # negative sizes
    assert _scan(L, n_bytes=-1) == _lib.GF_ERR_ARG
    assert _scan(L, max_len=-1) == _lib.GF_ERR_ARG
    assert _scan(L, hits_cap=-1) == _lib.GF_ERR_ARG
    assert _scan(L, ws_bytes=-5) == _lib.GF_ERR_ARG
    assert _scan(L, n_genes=-1) == _lib.GF_ERR_ARG
    assert _scan(L, max_len=_lib.GF_MAX_READ_LEN + 1) == _lib.GF_ERR_READ_TOO_LONG
    assert b"GF_MAX_READ_LEN" in L.gf_se_last_error()


def test_scan_single_device_raises_without_a_device():
    """No CPU fallback: host tensors (all there is without a GPU) are refused, and nothing is computed."""
    import torch
    from genefuserust_amd import Indexer, _lib
    from genefuserust_amd.single_end import scan_single_device
    ix = Indexer.from_gene_slices([b"ACGT" * 100])
    bases = torch.from_numpy(np.frombuffer(b"ACGT" * 40, dtype=np.uint8).copy())
    off = torch.tensor([0, 160], dtype=torch.int64)
    with pytest.raises(_lib.GfError) as e:
        scan_single_device(ix, bases, bases, off, 160)
    assert e.value.code == _lib.GF_ERR_NO_DEVICE


def test_gfmatch_sources_untouched():
    """The profiled library's sources and the three public headers stay byte-identical."""
    r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--verify", "-q", "main"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("no main branch in this checkout")
    d = subprocess.run(["git", "-C", ROOT, "diff", "main", "--", "genefuserust_amd/csrc", "include/gfmatch.h",
                        "include/gf_single_end.h", "include/gf_multi_csv.h"], capture_output=True, text=True)
    assert d.returncode == 0 and d.stdout == ""
