"""CPU-side checks of libgfnames.so, the names of a scan's hit records (include/gf_hit_names.h): it loads next to
libgfmatch.so, exports what its header declares, is bound by INTEGRATION.md, sizes its workspace sensibly, rejects bad
arguments before it touches a device, and has no CPU fallback.  Plus what the streamed file scans do without a device:
the byte sources hand out the files' bytes, and ``chunk_bytes`` is refused where nothing is streamed."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "gf_hit_names.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gf_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_entry_points():
    assert _declared_functions() == ["gf_hn_last_error", "gf_hn_names_device", "gf_hn_workspace_bytes"]


def test_library_exports_every_declared_symbol():
    from genefuserust_amd import hit_names
    L = hit_names.lib()
    for name in _declared_functions():
        assert hasattr(L, name), "libgfnames.so does not export %s" % name


def test_library_needs_libgfmatch_next_to_it():
    out = subprocess.run(["readelf", "-d", os.path.join(ROOT, "genefuserust_amd", "libgfnames.so")],
                         capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("readelf not available")
    assert "[libgfmatch.so]" in out.stdout and "$ORIGIN" in out.stdout


def test_integration_doc_binds_every_entry_point():
    """INTEGRATION.md's fourth `extern "C"` block (after the one of gf_multi_csv.h) binds every function of
    gf_hit_names.h."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = doc.index('extern "C" {', doc.index("pub fn gf_mc_last_error()"))
    block = doc[start:doc.index("}", start)]
    bound = set(re.findall(r"pub fn (gf_[a-z0-9_]+)\(", block))
    missing = [n for n in _declared_functions() if n not in bound]
    assert not missing, missing


def test_workspace_is_monotone_in_the_record_capacity():
    from genefuserust_amd import hit_names
    L = hit_names.lib()
    caps = [0, 1, 31, 32, 33, 1024, 4097, 65536, 1 << 20, 20_000_000]
    w = [L.gf_hn_workspace_bytes(c) for c in caps]
    assert all(a <= b for a, b in zip(w, w[1:])), w
    assert all(x >= 8 * c for x, c in zip(w, caps))   # a start per record at the very least
    assert L.gf_hn_workspace_bytes(-1) == 0


def _names(L, idx=None, hits_cap=10, l_text=True, l_bytes=100, l_nl=8, r_text=False, r_bytes=0, r_nl=0, ws_bytes=1 << 20,
           names_cap=64, totals=True, name_totals=True, off=True):
    buf = (C.c_char * 256)()
    dummy = C.cast(buf, C.c_void_p)
    return L.gf_hn_names_device(idx, dummy, dummy if totals else None, hits_cap, 0, dummy if l_text else None, l_bytes,
                                dummy, l_nl, dummy if r_text else None, r_bytes, dummy if r_text else None, r_nl, dummy,
                                ws_bytes, dummy, names_cap, dummy if off else None, dummy if name_totals else None, None)


def test_argument_errors_without_a_device():
    from genefuserust_amd import _lib, hit_names
    L = hit_names.lib()
    assert _names(L) == _lib.GF_ERR_ARG                                    # null index
    assert b"null index" in L.gf_hn_last_error()
    fake = C.cast((C.c_char * 64)(), C.c_void_p)   # (never dereferenced: the checks below come first)
    assert _names(L, fake, totals=False) == _lib.GF_ERR_ARG                 # null totals, the scan's and the names'
    assert _names(L, fake, name_totals=False) == _lib.GF_ERR_ARG
    assert b"totals" in L.gf_hn_last_error()
    assert _names(L, fake, off=False) == _lib.GF_ERR_ARG
    for neg in (dict(hits_cap=-1), dict(l_bytes=-1), dict(l_nl=-1), dict(r_bytes=-1), dict(r_nl=-1),
                dict(names_cap=-1), dict(ws_bytes=-5)):                     # negative sizes
        assert _names(L, fake, **neg) == _lib.GF_ERR_ARG, neg
        assert b"negative" in L.gf_hn_last_error()
    assert _names(L, fake, l_text=False) == _lib.GF_ERR_ARG                 # null text with records
    assert b"null text" in L.gf_hn_last_error()
    assert _names(L, fake, r_bytes=10) == _lib.GF_ERR_ARG                   # a size for R2 without R2
    assert _names(L, fake, ws_bytes=8) == _lib.GF_ERR_CAPACITY              # workspace too small
    assert b"gf_hn_workspace_bytes" in L.gf_hn_last_error()


def test_hit_names_device_raises_without_a_device():
    """No CPU fallback: host tensors (all there is without a GPU) are refused, and nothing is computed."""
    import torch
    from genefuserust_amd import Indexer, _lib
    from genefuserust_amd.fastq import FastqBatch
    from genefuserust_amd.hit_names import hit_names_device
    from genefuserust_amd.read_pair import PairScan
    ix = Indexer.from_gene_slices([b"ACGT" * 100])
    text = torch.from_numpy(np.frombuffer(b"@a\nACGT\n+\nFFFF\n", dtype=np.uint8).copy())
    nl = torch.tensor([2, 7, 9, 14], dtype=torch.int64)
    batch = FastqBatch(text, text, nl, 1, nl, 4, 0)
    scan = PairScan(torch.zeros((4, 64), dtype=torch.uint8), text, text, torch.zeros(8, dtype=torch.int64))
    with pytest.raises(_lib.GfError) as e:
        hit_names_device(ix, scan, text, batch)
    assert e.value.code == _lib.GF_ERR_NO_DEVICE


# ---- the byte sources ------------------------------------------------------------------------------------------------

def _drain(source, sizes):
    """Everything ``source.readinto`` hands out when it is asked for ``sizes`` bytes in turn (cyclically)."""
    out, k = bytearray(), 0
    while True:
        buf = bytearray(sizes[k % len(sizes)])
        n = source.readinto(memoryview(buf))
        assert 0 <= n <= len(buf)
        if n == 0:
            return bytes(out)
        out += buf[:n]
        k += 1


def test_byte_sources_hand_out_the_same_bytes(tmp_path):
    from genefuserust_amd.fastq import FastqReader
    from genefuserust_amd.scan_stream import ArraySource
    rng = np.random.default_rng(4)
    recs = []
    for k in range(400):
        n = int(rng.integers(1, 200))
        recs += [b"@read_%d some comment" % k, bytes(rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), n)), b"+",
                 bytes(rng.integers(33, 75, size=n, dtype=np.uint8))]
    text = b"\n".join(recs)   # (no final newline)
    plain, zipped, two = tmp_path / "a.fq", tmp_path / "a.fq.gz", tmp_path / "b.fastq.gz"
    plain.write_bytes(text)
    with gzip.open(zipped, "wb") as f:
        f.write(text)
    cut = len(text) // 3
    two.write_bytes(gzip.compress(text[:cut]) + gzip.compress(text[cut:]))   # two members, one after the other
    for sizes in ([1], [7, 1, 13], [997], [4096, 3], [len(text) + 5]):
        assert _drain(ArraySource(np.frombuffer(text, dtype=np.uint8).copy()), sizes) == text
        for path in (plain, zipped, two):
            with FastqReader(str(path)).open_stream() as s:
                assert s.name == str(path)
                assert _drain(s, sizes) == text, (path, sizes)
                assert s.readinto(memoryview(bytearray(8))) == 0   # the end stays the end
    assert FastqReader(str(two)).text() == text
    # an array also lends its bytes where they are
    a = ArraySource(np.frombuffer(text, dtype=np.uint8).copy())
    assert a.take(10).tobytes() == text[:10] and not a.at_end()
    assert a.take(len(text)).tobytes() == text[10:] and a.at_end() and a.take(5).size == 0


def test_chunk_bytes_is_refused_where_nothing_is_streamed(tmp_path):
    from genefuserust_amd.multi_csv_scan import scan_report
    from genefuserust_amd.scan import scan_single_end_files, scan_single_end_report
    with pytest.raises(ValueError, match="chunk_bytes"):
        scan_single_end_report("ref.fa", "f.csv", "r1.fq", route="host", chunk_bytes=1 << 20)
    with pytest.raises(ValueError, match="chunk_bytes"):
        scan_single_end_files("ref.fa", "f.csv", "r1.fq", route="host", chunk_bytes=1 << 20)
    with pytest.raises(ValueError, match="chunk_bytes"):     # a list of CSVs: multi-CSV mode keeps its reads resident
        scan_report("ref.fa", str(tmp_path / "panels.txt"), "r1.fq", "r2.fq", chunk_bytes=1 << 20)
    with pytest.raises(ValueError, match="chunk_bytes"):
        scan_report("ref.fa", str(tmp_path / "panels.txt"), "r1.fq", chunk_bytes=1 << 20)


def test_existing_public_headers_and_gfmatch_sources_untouched():
    """The new library is an added one: csrc/ and the three earlier public headers stay byte-identical."""
    r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--verify", "-q", "main"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("no main branch in this checkout")
    d = subprocess.run(["git", "-C", ROOT, "diff", "main", "--", "genefuserust_amd/csrc", "include/gfmatch.h",
                        "include/gf_single_end.h", "include/gf_multi_csv.h"], capture_output=True, text=True)
    assert d.returncode == 0 and d.stdout == ""
