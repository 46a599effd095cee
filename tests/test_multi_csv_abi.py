"""CPU-side checks of libgfmcsv.so, the paired-end scan of multi-CSV mode (include/gf_multi_csv.h), and of the
file-level helpers of genefuserust_amd/multi_csv_scan.py: the library loads next to libgfmatch.so, exports what its
header declares, is bound by INTEGRATION.md, sizes its buffers sensibly, rejects bad arguments before it touches a
device and has no CPU fallback; the list file, the report names and the mode switch follow fusion_scan.rs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FUNCTIONS = ["gf_mc_last_error", "gf_mc_pairs_prepare_device", "gf_mc_pairs_scan_device", "gf_mc_prepared_bytes",
             "gf_mc_retry_capacity", "gf_mc_scan_workspace_bytes"]


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "gf_multi_csv.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gf_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_entry_points():
    assert _declared_functions() == FUNCTIONS


def test_library_exports_every_declared_symbol():
    from genefuserust_amd import multi_csv_scan
    L = multi_csv_scan.lib()
    for name in FUNCTIONS:
        assert hasattr(L, name), "libgfmcsv.so does not export %s" % name


def test_library_needs_libgfmatch_next_to_it():
    out = subprocess.run(["readelf", "-d", os.path.join(ROOT, "genefuserust_amd", "libgfmcsv.so")], capture_output=True,
                         text=True)
    assert out.returncode == 0, out.stderr
    assert "[libgfmatch.so]" in out.stdout and "$ORIGIN" in out.stdout


def test_integration_doc_binds_every_entry_point():
    """INTEGRATION.md's third `extern "C"` block (after the one of gf_single_end.h) binds every function of
    gf_multi_csv.h."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = doc.index('extern "C" {', doc.index("pub fn gf_se_last_error()"))
    block = doc[start:doc.index("}", start)]
    bound = set(re.findall(r"pub fn (gf_[a-z0-9_]+)\(", block))
    assert bound == set(FUNCTIONS)


def test_sizes_are_monotone_with_floors():
    from genefuserust_amd import _lib, multi_csv_scan
    L = multi_csv_scan.lib()
    ns = [0, 1, 100, 255, 256, 257, 4096, 65536, 1 << 20, 10_000_000]
    for max_len in (1, 150, 300, 2048):
        for rc in (0, 1, 17, 4096, 1 << 20):
            w = [L.gf_mc_scan_workspace_bytes(n, max_len, rc) for n in ns]
            assert all(a <= b for a, b in zip(w, w[1:])), (max_len, rc, w)
        for n in ns:
            w = [L.gf_mc_scan_workspace_bytes(n, max_len, rc) for rc in (1, 2, 100, 4096, 1 << 20, 1 << 30)]
            assert all(a <= b for a, b in zip(w, w[1:])), (max_len, n, w)
    # per pair at the very least: three counts, three pairs of matches, three status bytes
    n = 1 << 20
    assert L.gf_mc_scan_workspace_bytes(n, 150, 1) >= n * (3 + 3 * 32 + 3)
    assert L.gf_mc_scan_workspace_bytes(n, 150, 0) >= L.gf_mc_scan_workspace_bytes(n, 150, 1)
    for k in (0, 1, 1000, 4096, 100_000, 10_000_000):
        assert L.gf_mc_retry_capacity(k) >= 4096
    assert L.gf_mc_retry_capacity(10_000_000) >= 10_000_000 // 32
    assert L.gf_mc_retry_capacity(-1) == 0
    assert L.gf_mc_scan_workspace_bytes(-1, 150, 0) == 0 and L.gf_mc_scan_workspace_bytes(10, -1, 0) == 0
    # the prepared buffer: monotone in the pairs and in the bytes; the per-pair arrays (merged length, diff, place:
    # 12 bytes), three offsets per pair, the reads themselves and their packed form (6 bytes per 16 bases)
    p = [L.gf_mc_prepared_bytes(k, 150 * k, 150 * k, 150) for k in ns]
    assert all(a <= b for a, b in zip(p, p[1:])), p
    b = [L.gf_mc_prepared_bytes(1000, x, 150_000, 150) for x in (0, 1, 1000, 150_000, 10 ** 9)]
    assert all(a <= c for a, c in zip(b, b[1:])), b
    n, nb = 1 << 20, 150 << 20
    assert L.gf_mc_prepared_bytes(n, nb, nb, 150) >= n * 12 + 3 * 8 * n + 2 * nb + _lib.lib().gf_packed_chunks(2 * nb) * 6
    for bad in ((-1, 10, 10, 150), (10, -1, 10, 150), (10, 10, -1, 150), (10, 10, 10, -1)):
        assert L.gf_mc_prepared_bytes(*bad) == 0


_BUF = (C.c_char * 64)()
_P = C.cast(_BUF, C.c_void_p)


def _prepare(L, idx=None, n=10, l_bytes=1500, r_bytes=1500, max_len=150, prepared=_P, prepared_bytes=1 << 30):
    return L.gf_mc_pairs_prepare_device(idx, _P, _P, _P, l_bytes, _P, _P, _P, r_bytes, n, max_len, prepared,
                                        prepared_bytes, None)


def _scan(L, idx=None, n=10, l_bytes=1500, r_bytes=1500, max_len=150, n_genes=0, ws_bytes=1 << 30, hits_cap=0,
          bytes_cap=0, totals=True):
    return L.gf_mc_pairs_scan_device(idx, _P, _P, _P, _P, l_bytes, _P, _P, _P, r_bytes, n, max_len, None, n_genes, 0, 0,
                                     _P, ws_bytes, None, hits_cap, None, None, bytes_cap, _P if totals else None, None)


def test_argument_errors_without_a_device():
    from genefuserust_amd import _lib, multi_csv_scan
    L = multi_csv_scan.lib()
    for call in (_prepare, _scan):
        assert call(L) == _lib.GF_ERR_ARG                                  # null index
        assert b"null index" in L.gf_mc_last_error()
        assert call(L, n=-1) == _lib.GF_ERR_ARG                            # negative sizes
        assert call(L, l_bytes=-1) == _lib.GF_ERR_ARG
        assert call(L, r_bytes=-1) == _lib.GF_ERR_ARG
        assert call(L, max_len=-1) == _lib.GF_ERR_ARG
        assert call(L, max_len=_lib.GF_MAX_READ_LEN // 2 + 1) == _lib.GF_ERR_READ_TOO_LONG
        assert b"GF_MAX_READ_LEN" in L.gf_mc_last_error()
    assert _prepare(L, prepared_bytes=-1) == _lib.GF_ERR_ARG
    assert _scan(L, ws_bytes=-5) == _lib.GF_ERR_ARG
    assert _scan(L, n_genes=-1) == _lib.GF_ERR_ARG
    assert _scan(L, hits_cap=-1) == _lib.GF_ERR_ARG
    assert _scan(L, bytes_cap=-1) == _lib.GF_ERR_ARG


def test_capacity_and_null_totals_are_checked_before_the_device():
    """The checks that come after the null-index check, with an index pointer that nothing dereferences before them:
    a short workspace or prepared buffer is GF_ERR_CAPACITY and null totals GF_ERR_ARG — returned although the
    'index' is not one, so nothing looked at it, let alone at a device."""
    from genefuserust_amd import _lib, multi_csv_scan
    L = multi_csv_scan.lib()
    fake = _P
    assert _scan(L, idx=fake, totals=False) == _lib.GF_ERR_ARG
    assert b"null totals" in L.gf_mc_last_error()
    assert _scan(L, idx=fake, ws_bytes=L.gf_mc_scan_workspace_bytes(10, 150, 0) - 1) == _lib.GF_ERR_CAPACITY
    assert _scan(L, idx=fake, ws_bytes=0) == _lib.GF_ERR_CAPACITY
    assert _prepare(L, idx=fake, prepared_bytes=L.gf_mc_prepared_bytes(10, 1500, 1500, 150) - 1) == _lib.GF_ERR_CAPACITY
    assert _prepare(L, idx=fake, prepared=None) == _lib.GF_ERR_CAPACITY
    assert _scan(L, idx=fake, n=(1 << 31) // 3 + 1) == _lib.GF_ERR_CAPACITY
    assert _scan(L, idx=fake, hits_cap=4) == _lib.GF_ERR_ARG             # room for hits asked, no buffer given
    assert _scan(L, idx=fake, n_genes=3) == _lib.GF_ERR_ARG              # gene flags missing


def test_host_tensors_are_refused():
    """No CPU fallback: host tensors (all there is without a GPU) are refused, and nothing is computed."""
    import torch
    from genefuserust_amd import Indexer, _lib
    from genefuserust_amd.multi_csv_scan import prepare_pairs_device
    ix = Indexer.from_gene_slices([b"ACGT" * 100])
    bases = torch.from_numpy(np.frombuffer(b"ACGT" * 40, dtype=np.uint8).copy())
    off = torch.tensor([0, 160], dtype=torch.int64)
    with pytest.raises(_lib.GfError) as e:
        prepare_pairs_device(ix, bases, bases, off, bases, bases, off, 160)
    assert e.value.code == _lib.GF_ERR_NO_DEVICE


def test_other_libraries_untouched():
    """The profiled library's sources and the three public headers stay byte-identical."""
    r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--verify", "-q", "main"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("no main branch in this checkout")
    d = subprocess.run(["git", "-C", ROOT, "diff", "main", "--", "genefuserust_amd/csrc", "include/gfmatch.h",
                        "include/gf_single_end.h", "include/gf_multi_csv.h"], capture_output=True, text=True)
    assert d.returncode == 0 and d.stdout == ""


# ---- the list file, the report names, the mode switch ------------------------------------------------------------

def test_read_csv_list(tmp_path):
    from genefuserust_amd.multi_csv_scan import read_csv_list
    a, b = tmp_path / "a.csv", tmp_path / "b panel.csv"
    a.write_text(">A_1,chr1:1-2\n")
    b.write_text(">B_1,chr1:1-2\n")
    lst = tmp_path / "panels.txt"
    lst.write_text("%s\n\n   \n  %s  \n\t%s\r\n%s" % (b, a, b, a))       # blank lines, blanks around, no last newline
    assert read_csv_list(str(lst)) == [str(b), str(a), str(b), str(a)]    # order and duplicates kept
    empty = tmp_path / "empty.txt"
    empty.write_text("\n\n")
    assert read_csv_list(str(empty)) == []
    lst.write_text("%s\n%s\n" % (a, tmp_path / "missing.csv"))
    with pytest.raises(FileNotFoundError) as e:
        read_csv_list(str(lst))
    assert "missing.csv" in str(e.value)
    lst.write_text("%s\n%s\n" % (a, "x" * 1001))
    with pytest.raises(ValueError):
        read_csv_list(str(lst))
    with pytest.raises(FileNotFoundError):
        read_csv_list(str(tmp_path / "no_such_list.txt"))


def test_report_names():
    """Expected strings by hand from fusion_scan.rs:190-251: [parent, "{stem}_{csvstem}.{ext}"] joined as a PathBuf,
    stem and extension split at the LAST dot of the file name."""
    from genefuserust_amd.multi_csv_scan import report_names
    csvs = ["/data/panels/druggable.csv", "cancer.hg38.csv", "rel/dir/x.csv"]
    assert report_names("out/run1.json", csvs) == ["out/run1_druggable.json", "out/run1_cancer.hg38.json",
                                                   "out/run1_x.json"]
    assert report_names("report.json", csvs) == ["report_druggable.json", "report_cancer.hg38.json", "report_x.json"]
    assert report_names("/abs/s1.v2.html", csvs[:2]) == ["/abs/s1.v2_druggable.html", "/abs/s1.v2_cancer.hg38.html"]
    assert report_names("", csvs) == []
    assert report_names("out/run1.json", []) == []
    assert report_names("r.json", ["a.csv", "d/a.csv"]) == ["r_a.json", "r_a.json"]   # same stem: the same name
    with pytest.raises(ValueError):
        report_names("no_extension", csvs)


def test_scan_report_dispatches_on_the_extension(monkeypatch):
    from genefuserust_amd import multi_csv_scan, scan
    calls = []
    monkeypatch.setattr(scan, "scan_pair_end_report",
                        lambda *a, **k: (calls.append(("pe", a)) or (["pe"], {"fusions": 1})))
    monkeypatch.setattr(scan, "scan_single_end_report",
                        lambda *a, **k: (calls.append(("se", a)) or (["se"], {"fusions": 1})))
    monkeypatch.setattr(multi_csv_scan, "scan_multi_csv_report",
                        lambda *a, **k: (calls.append(("multi", a)) or [("x.csv", [], {})]))
    assert multi_csv_scan.scan_report("ref.fa", "p.csv", "r1.fq", "r2.fq") == (["pe"], {"fusions": 1})
    assert calls[-1][0] == "pe" and calls[-1][1][:4] == ("ref.fa", "p.csv", "r1.fq", "r2.fq")
    assert multi_csv_scan.scan_report("ref.fa", "dir.v1/p.csv", "r1.fq") == (["se"], {"fusions": 1})
    assert calls[-1][0] == "se" and calls[-1][1][:3] == ("ref.fa", "dir.v1/p.csv", "r1.fq")
    for name in ("panels.txt", "panels.list", "panels.csv.txt", "panels.CSV"):   # the match is on "csv" exactly
        assert multi_csv_scan.scan_report("ref.fa", name, "r1.fq", "r2.fq") == [("x.csv", [], {})]
        assert calls[-1][0] == "multi" and calls[-1][1][:4] == ("ref.fa", name, "r1.fq", "r2.fq")
    assert len(calls) == 6
