"""gf_hn_records_device of libgfnames.so (include/gf_hit_records.h) on the device: the original FASTQ records of hand-made
hit records, span by span against ``fastq.record_lines`` of the host text — and, where a last record is cut short and
``record_lines`` has no line to cut, against the lines of the host text themselves."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_stream_files import _device_text, _golden_index, _scan_of

SCAN_TOTALS_THREADS = 1024   # GF_SCAN_TOTALS_THREADS: one element per scan thread up to here


# ---- without a device ----------------------------------------------------------------------------------------------

def test_header_and_library_agree():
    from genefuserust_amd import hit_names
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gf_hit_records.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(gf_[a-z0-9_]+)\s*\(", src)))
    assert declared == ["gf_hn_records_device", "gf_hn_records_workspace_bytes"]
    L = hit_names.lib()
    assert all(hasattr(L, name) for name in declared)
    caps = [0, 1, 63, 64, 1025, 1 << 20, 20_000_000]
    w = [L.gf_hn_records_workspace_bytes(c) for c in caps]
    assert all(a <= b for a, b in zip(w, w[1:])) and all(x >= 16 * c for x, c in zip(w, caps))   # a start per span
    assert L.gf_hn_records_workspace_bytes(-1) == 0


def test_argument_errors_without_a_device():
    from genefuserust_amd import _lib, hit_names
    L = hit_names.lib()
    dummy = C.cast((C.c_char * 256)(), C.c_void_p)

    def call(idx=dummy, hits_cap=10, l_text=dummy, l_bytes=100, r_text=None, r_bytes=0, ws_bytes=1 << 20, cap=64, off=dummy,
             totals=dummy):
        return L.gf_hn_records_device(idx, dummy, dummy, hits_cap, 0, l_text, l_bytes, dummy, 8, r_text, r_bytes,
                                      r_text, 0, dummy, ws_bytes, dummy, cap, off, totals, None)
    assert call(idx=None) == _lib.GF_ERR_ARG and b"null index" in L.gf_hn_last_error()
    assert call(totals=None) == _lib.GF_ERR_ARG and call(off=None) == _lib.GF_ERR_ARG
    for neg in (dict(hits_cap=-1), dict(l_bytes=-1), dict(r_bytes=-1), dict(cap=-1), dict(ws_bytes=-5)):
        assert call(**neg) == _lib.GF_ERR_ARG and b"negative" in L.gf_hn_last_error(), neg
    assert call(l_text=None) == _lib.GF_ERR_ARG and b"null text" in L.gf_hn_last_error()
    assert call(r_bytes=10) == _lib.GF_ERR_ARG                       # a size for R2 without R2
    assert call(ws_bytes=L.gf_hn_records_workspace_bytes(10) - 1) == _lib.GF_ERR_CAPACITY
    assert b"gf_hn_records_workspace_bytes" in L.gf_hn_last_error()


def test_hit_records_device_raises_without_a_device():
    """No CPU fallback: host tensors are refused, and nothing is computed."""
    import torch
    from genefuserust_amd import Indexer, _lib
    from genefuserust_amd.fastq import FastqBatch
    from genefuserust_amd.hit_names import hit_records_device
    from genefuserust_amd.read_pair import PairScan
    ix = Indexer.from_gene_slices([b"ACGT" * 100])
    text = torch.from_numpy(np.frombuffer(b"@a\nACGT\n+\nFFFF\n", dtype=np.uint8).copy())
    nl = torch.tensor([2, 7, 9, 14], dtype=torch.int64)
    scan = PairScan(torch.zeros((4, 64), dtype=torch.uint8), text, text, torch.zeros(8, dtype=torch.int64))
    with pytest.raises(_lib.GfError) as e:
        hit_records_device(ix, scan, text, FastqBatch(text, text, nl, 1, nl, 4, 0))
    assert e.value.code == _lib.GF_ERR_NO_DEVICE


# ---- on the device ---------------------------------------------------------------------------------------------------

def _host_record(text: bytes, i: int):
    """(name, sequence, strand, quality) of record i from the lines of the host text, None when i is off the text."""
    if i < 0 or i > text.count(b"\n") // 4:
        return None
    return tuple((text.split(b"\n")[4 * i:4 * i + 4] + [b""] * 4)[:4])


def _host_span(text: bytes, i: int) -> bytes:
    if _host_record(text, i) is None:
        return b""
    return b"\n".join(text.split(b"\n")[4 * i:4 * i + 4])


def _check(ix, texts, ids, base=0, cap=None, records_cap=None):
    """Gathers the records of ``ids`` ((FASTQ record, source) pairs) from ``texts`` ((R1, R2) or (reads,)) and holds
    every span, offset and total to the host text; whole records also to ``record_lines``."""
    from genefuserust_amd.fastq import fastq_cut_device, record_lines
    from genefuserust_amd.hit_names import hit_records_device
    dev = [_device_text(t) for t in texts]
    batches = [fastq_cut_device(ix, d) for d in dev]
    scan = _scan_of(ids, cap=cap, base=base)
    args = [x for pair in zip(dev, batches) for x in pair]
    rec = hit_records_device(ix, scan, *args, pair_id_base=base, records_cap=records_cap)
    n = min(len(ids), cap or len(ids))
    S = len(texts)
    assert rec.sides == S
    want = [[_host_record(t, i) or (b"",) * 4 for t in texts] for i, _ in ids[:n]]
    spans = [_host_span(t, i) for i, _ in ids[:n] for t in texts]
    missing = sum(1 for i, _ in ids[:n] for t in texts if _host_record(t, i) is None)
    assert [int(x) for x in rec.totals.cpu()] == [S * n, sum(len(s) for s in spans), 0, missing]
    off = rec.offsets[:S * n + 1].cpu().numpy()
    assert off[0] == 0 and (np.diff(off) == [len(s) for s in spans]).all()
    assert rec.records[:int(off[-1])].cpu().numpy().tobytes() == b"".join(spans)
    got = rec.download()
    assert got == [[tuple(r) for r in w] for w in want]
    for (i, _), g in zip(ids[:n], got):
        for s, (b, t) in enumerate(zip(batches, texts)):
            if 0 <= i < b.n_records:
                assert g[s] == record_lines(b, t, i), (i, s)
    return got


def _pair_texts(n, final_newline=(True, False), r2_extra=7):
    r1 = b"\n".join(b"@p%d/1 x\n%s\n+\n%s" % (k, b"ACGT" * (k % 5 + 1), b"F" * (4 * (k % 5 + 1))) for k in range(n))
    r2 = b"\n".join(b"@pair_%d/2 with a comment\n%s\n+\n%s" % (k, b"TG" * (k % 7 + r2_extra), b"#" * (2 * (k % 7 + r2_extra)))
                    for k in range(n))
    return r1 + (b"\n" if final_newline[0] else b""), r2 + (b"\n" if final_newline[1] else b"")


@pytest.mark.gpu
def test_basic_gathers(gpu_device):
    ix, _ = _golden_index()
    t1, t2 = _pair_texts(9)
    # record 0, the last one, a pair hit twice, every source: both sides are gathered regardless
    ids = [(0, 1), (8, 2), (3, 0), (3, 1), (3, 2), (5, 0), (0, 2)]
    got = _check(ix, (t1, t2), ids)
    assert got[0][0][0] == b"@p0/1 x" and got[1][1][0] == b"@pair_8/2 with a comment"
    assert got[2] == got[3] == got[4] and got[0] == got[6]
    assert all(len(g) == 2 and g[0][2] == g[1][2] == b"+" for g in got)
    _check(ix, (t1, t2), ids, base=7_000_000_123)
    # single-end: one span per record, whatever its source
    got = _check(ix, (t1,), ids, base=11)
    assert all(len(g) == 1 for g in got) and got[1][0][0] == b"@p8/1 x"
    ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("final_newline", [True, False])
def test_text_shapes(gpu_device, final_newline):
    ix, _ = _golden_index()
    end = b"\n" if final_newline else b""
    # spans of 63, 64, 65 and 129 bytes and one over 1000 cross the lane stride; empty lines inside a record; R2's
    # records of other lengths than R1's
    def record(name_len, seq_len):
        return b"@" + b"n" * (name_len - 1) + b"\n" + b"A" * seq_len + b"\n+\n" + b"I" * seq_len
    sized = [record(10, (size - 10 - 4) // 2) + (b"" if (size - 10) % 2 == 0 else b"J") for size in (63, 64, 65, 129)]
    assert [len(s) for s in sized] == [63, 64, 65, 129]
    long_one = record(40, 520)
    assert len(long_one) > 1000
    t1 = b"\n".join(sized + [long_one, b"@empty lines\n\n+\n", b"\n\n\n", b"@last\nAC\n+\nFF"]) + end
    t2 = b"\n".join([long_one, b"@b\nA\n+\nF", record(5, 33), b"\n\n\n", record(70, 150), b"@x\n\n\n", b"@y\nAC\n+\n!!",
                     b"@last/2\nACGTA\n+\nFFFFF"]) + end
    ids = [(k, k % 3) for k in range(8)]
    got = _check(ix, (t1, t2), ids)
    assert got[5][0] == (b"@empty lines", b"", b"+", b"") and got[6][0] == (b"", b"", b"", b"")
    assert got[4][0][1] == b"A" * 520 and got[0][1][1] == b"A" * 520
    ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cut", [b"@cut", b"@cut\n", b"@cut\nACGT", b"@cut\nACGT\n", b"@cut\nACGT\n+", b"@cut\nACGT\n+\n"])
def test_last_record_cut_short(gpu_device, cut):
    """A last record cut after 1, 2 and 3 lines, with and without the line's newline: the span runs to the end of the
    text, and the missing lines are empty."""
    ix, _ = _golden_index()
    t1 = b"@a/1\nACGT\n+\nFFFF\n@b/1\nAC\n+\nFF\n" + cut
    t2 = b"@a/2\nTTTT\n+\nFFFF\n@b/2\nTT\n+\nFF\n@whole/2\nAAA\n+\nFFF\n"
    got = _check(ix, (t1, t2), [(2, 1), (1, 0), (2, 2)])
    lines = cut.split(b"\n")
    assert got[0][0] == tuple((lines + [b""] * 4)[:4]) and got[0][1] == (b"@whole/2", b"AAA", b"+", b"FFF")
    assert got[2] == got[0] and got[1][0] == (b"@b/1", b"AC", b"+", b"FF")
    ix.close()


@pytest.mark.gpu
def test_records_off_the_text(gpu_device):
    from genefuserust_amd.hit_names import hit_records_device
    from genefuserust_amd.fastq import fastq_cut_device
    ix, _ = _golden_index()
    t1, t2 = _pair_texts(6, r2_extra=1)
    t2 = b"\n".join(t2.split(b"\n")[:16])   # R2 has four records only
    base = 5_000_000_000
    # past both texts, before pair_id_base, past R2 only (one span of the two is missing)
    ids = [(0, 1), (9, 1), (-1, 2), (5, 0), (-4_000_000_000, 1), (1 << 40, 2), (3, 2)]
    got = _check(ix, (t1, t2), ids, base=base)
    assert got[1] == got[2] == [(b"",) * 4] * 2 and got[3][1] == (b"",) * 4 and got[3][0][0] == b"@p5/1 x"
    _check(ix, (t1,), ids, base=base)
    # hits_cap below totals[0]: the capacity's records only
    d1, d2 = _device_text(t1), _device_text(t2)
    b1, b2 = fastq_cut_device(ix, d1), fastq_cut_device(ix, d2)
    scan = _scan_of([(0, 1), (1, 1), (2, 1)])
    scan.totals[0] = 1000   # (the scan found more than it had room for)
    rec = hit_records_device(ix, scan, d1, b1, d2, b2)
    assert [r[0][0] for r in rec.download()] == [b"@p0/1 x", b"@p1/1 x", b"@p2/1 x"]
    assert int(rec.totals[0].item()) == 6
    # zero records: a capacity, but totals[0] == 0; and no capacity at all
    empty = _scan_of([], cap=8)
    for scan in (empty, empty._replace(hits=empty.hits[:0])):
        rec = hit_records_device(ix, scan, d1, b1, d2, b2)
        assert rec.download() == [] and [int(x) for x in rec.totals.cpu()] == [0, 0, 0, 0]
        assert int(rec.offsets[0].item()) == 0
    ix.close()


@pytest.mark.gpu
def test_records_capacity_one_byte_too_small(gpu_device):
    """The overflow bit, the true offsets and byte count, every span that fits where it belongs, the one that does not
    untouched, the retry with the bytes asked for; and a workspace one byte short."""
    import torch
    from genefuserust_amd import _lib
    from genefuserust_amd.fastq import fastq_cut_device
    from genefuserust_amd.hit_names import HitRecords, hit_records_device, lib
    ix, _ = _golden_index()
    t1, t2 = _pair_texts(40)
    d1, d2 = _device_text(t1), _device_text(t2)
    b1, b2 = fastq_cut_device(ix, d1), fastq_cut_device(ix, d2)
    ids = [(k, k % 3) for k in range(0, 40, 3)]
    spans = [_host_span(t, i) for i, _ in ids for t in (t1, t2)]
    need = sum(len(s) for s in spans)
    scan = _scan_of(ids)
    cap, guard = need - 1, 4096
    out = torch.full((cap + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    off = torch.zeros(2 * len(ids) + 1, dtype=torch.int64, device="cuda")
    tot = torch.zeros(4, dtype=torch.int64, device="cuda")
    L = lib()
    ws_bytes = int(L.gf_hn_records_workspace_bytes(len(ids)))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")

    def call(ws_given, cap_given):
        return L.gf_hn_records_device(ix._handle(), scan.hits.data_ptr(), scan.totals.data_ptr(), len(ids), 0,
                                      d1.data_ptr(), d1.numel(), b1.nl_pos.data_ptr(), b1.n_newlines, d2.data_ptr(),
                                      d2.numel(), b2.nl_pos.data_ptr(), b2.n_newlines, ws.data_ptr(), ws_given,
                                      out.data_ptr(), cap_given, off.data_ptr(), tot.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    assert call(ws_bytes - 1, cap) == _lib.GF_ERR_CAPACITY        # (refused before the device is touched)
    assert b"gf_hn_records_workspace_bytes" in L.gf_hn_last_error()
    assert call(ws_bytes, cap) == _lib.GF_OK
    torch.cuda.synchronize()
    assert [int(x) for x in tot.cpu()] == [2 * len(ids), need, 1, 0]
    o = off.cpu().numpy()
    assert (np.diff(o) == [len(s) for s in spans]).all() and o[-1] == need   # the offsets are the true ones
    got = out.cpu().numpy().tobytes()
    assert got[:o[-2]] == b"".join(spans[:-1])                  # every span that fits
    assert got[o[-2]:] == b"\xa5" * (len(got) - o[-2])          # the last one is not started, the guard untouched
    with pytest.raises(_lib.GfError) as e:
        HitRecords(out[:cap], off, tot, 2).download()
    assert e.value.code == _lib.GF_ERR_CAPACITY and str(need) in str(e.value)
    # with the bytes it asked for
    again = hit_records_device(ix, scan, d1, b1, d2, b2, records_cap=int(tot[1].item())).download()
    assert [b"\n".join(r) for rec in again for r in rec] == spans
    ix.close()


@pytest.mark.gpu
def test_scan_past_one_element_per_scan_thread(gpu_device):
    """1500 short pair records: 3000 spans, three to a scan thread and the last threads idle.  The offsets equal the
    host's cumulative sum, and every span lies where they say."""
    ix, _ = _golden_index()
    n = 1500
    assert 2 * n > 2 * SCAN_TOTALS_THREADS and (2 * n) % SCAN_TOTALS_THREADS != 0
    t1, t2 = _pair_texts(n)
    rng = np.random.default_rng(8)
    ids = [(int(i), k % 3) for k, i in enumerate(rng.integers(0, n, size=n))]
    _check(ix, (t1, t2), ids)
    ix.close()
