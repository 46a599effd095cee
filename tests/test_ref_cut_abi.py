"""libgfrefcut.so on the device (include/gf_ref_cut.h): gf_rc_index_device and gf_rc_gather_device on crafted texts of a
few tiles, against the host loop of tests/test_ref_cut_plan.py (``model_index``, ``model_gather``), every field and
every output byte."""
import ctypes as C

import numpy as np
import pytest

from tests.test_ref_cut_plan import KEEP, model_gather, model_index

FILL = 0xEE


def _tile():
    from genefuserust_amd.ref_cut import tile_bytes
    return tile_bytes()


def _body(rng, nbytes: int, eol: bytes = b"\n") -> bytearray:
    """FASTA-like text: records of a dozen lines of 60 letters, lower case, '-', '*' and digits among them."""
    alphabet = np.frombuffer(b"ACGTACGTACGTacgtnN-*7", dtype=np.uint8)
    out, k = bytearray(), 0
    while len(out) < nbytes:
        out += b">contig%d some description %d" % (k, k) + eol
        for _ in range(12):
            out += bytes(rng.choice(alphabet, 60)) + eol
        k += 1
    return out[:nbytes]


def _device(text: bytes, head: int):
    """``text`` in HBM, ``head`` bytes behind a 16-byte boundary."""
    import torch
    buf = torch.full((head + len(text) + 1,), ord(">"), dtype=torch.uint8)   # ('>' around the text: not to be seen)
    buf[head:head + len(text)] = torch.from_numpy(np.frombuffer(bytes(text), dtype=np.uint8).copy())
    d = buf.cuda()
    assert d.data_ptr() % 16 == 0
    return d[head:head + len(text)]


def _check_index(text: bytes, head: int, cap_records: int = 256, names_cap: int = 1 << 14):
    from genefuserust_amd.ref_cut import lib, ref_index_device
    text = bytes(text)
    d = _device(text, head)
    ix = ref_index_device(d, cap_records, names_cap)
    got, want = ix.download(), model_index(text)
    assert (got.n, got.kept, got.unfinished) == (want.n, want.kept, want.unfinished)
    for f in ("gt_pos", "gt_rank", "name_end", "seq_rank"):
        assert getattr(got, f).tolist() == getattr(want, f).tolist(), f
    assert got.names == want.names
    # the kept rank at the start of every tile: the tiles lie on the grid of addresses
    T = _tile()
    ntiles = (head + len(text) + T - 1) // T if text else 0
    assert ntiles <= lib().gf_rc_tiles(len(text))
    rank = np.concatenate([[0], np.cumsum([c in KEEP for c in text])])
    want_tiles = [int(rank[max(t * T - head, 0)]) for t in range(ntiles)] + [int(rank[-1])]
    assert ix.tile_kept[:ntiles + 1].cpu().tolist() == want_tiles
    return d, ix, got


def _check_gather(text: bytes, d, ix, rec, rows, carried: int = 0, n_records=None, nbytes=None):
    import torch
    from genefuserust_amd.ref_cut import ref_gather_device
    n_records = rec.n if n_records is None else n_records
    nbytes = len(text) if nbytes is None else nbytes
    total = max((r[3] + r[2] - r[1] for r in rows), default=0) + 8
    out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    ref_gather_device(d[:nbytes], ix, n_records, rows, total, carried, out=out)
    got = out.cpu().numpy().tobytes()
    want = model_gather(bytes(text)[:nbytes], rec, n_records, rows, total, carried, fill=FILL)
    assert got == want
    return got


def _whole_records(rec, kept: int, carried: int = 0):
    """Rows that ask for every sequence byte of every record of a chunk, the carried-in one included."""
    ends = rec.gt_rank.tolist() + [kept]
    starts = [0] + rec.seq_rank.tolist()
    rows, off = [], 0
    for k, (s, e) in enumerate(zip(starts, ends)):
        lo = carried if k == 0 else 0
        if e > s:
            rows.append((k, lo, lo + e - s, off))
            off += e - s
    return rows


CASES = ["gt_last_of_tile", "gt_first_of_tile", "gt_before_last", "gt_second", "gt_all_four", "gt_ends_text",
         "delimiter_in_next_tile", "crlf", "inner_gt_and_description", "empty_record", "text_before_first",
         "no_gt", "no_final_newline", "tiny", "one_byte", "empty"]


def _case(name: str, head: int) -> bytes:
    T = _tile()
    rng = np.random.default_rng(CASES.index(name))
    t = _body(rng, 3 * T + 517)
    at = lambda grid: grid - head   # the text byte at a place on the grid of addresses
    if name.startswith("gt_") and name != "gt_ends_text":
        for g in {"gt_last_of_tile": [T - 1], "gt_first_of_tile": [T], "gt_before_last": [2 * T - 2],
                  "gt_second": [2 * T + 1], "gt_all_four": [T - 2, T - 1, T, T + 1]}[name]:
            t[at(g)] = ord(">")
    elif name == "gt_ends_text":
        t[-1] = ord(">")
    elif name == "delimiter_in_next_tile":
        t[at(T - 5):at(T + 70)] = b">a_name_across_the_tiles" + b"x" * 51
        t[at(T + 70)] = ord("\n")
    elif name == "crlf":
        t = _body(rng, 3 * T + 517, b"\r\n")
    elif name == "inner_gt_and_description":
        t[at(T - 40):at(T + 20)] = b">outer description of it>inner more words here ACGT\nACGTACG"
    elif name == "empty_record":
        t[at(2 * T - 1):at(2 * T + 2)] = b">\n>"
    elif name == "text_before_first":
        t = bytearray(b"ACGT no record yet\nACGTACGT\n" * 20) + t
    elif name == "no_gt":
        t = bytearray(bytes(t).replace(b">", b"A"))
    elif name == "no_final_newline":
        t = t[:bytes(t).rindex(b"\n")] + b"ACGTAC"
    elif name == "tiny":
        t = bytearray(b"x>a b\nAC-*gt9\n>\n>c")
    elif name == "one_byte":
        t = bytearray(b">")
    elif name == "empty":
        t = bytearray()
    return bytes(t)


@pytest.mark.gpu
@pytest.mark.parametrize("head", [0, 5, 15])
@pytest.mark.parametrize("name", CASES)
def test_index_and_gather_of_crafted_texts_equal_the_host_loop(gpu_device, name, head):
    text = _case(name, head)
    d, ix, rec = _check_index(text, head)
    if name in ("gt_all_four", "empty_record", "tiny"):
        assert b"" in rec.names
    if name in ("gt_ends_text", "one_byte"):
        assert rec.unfinished == len(text) - 1
    if name == "no_gt":
        assert rec.n == 0 and rec.kept > 0
    if name == "delimiter_in_next_tile":
        assert b"a_name_across_the_tiles" + b"x" * 51 in rec.names
    # every sequence byte of every record, the bytes in front of the first '>' as a record carried in with 1234 kept
    rows = _whole_records(rec, rec.kept, carried=1234)
    got = _check_gather(text, d, ix, rec, rows, carried=1234)
    assert len(rows) > 0 or name in ("one_byte", "empty")
    assert FILL not in got[:-8] and got[-8:] == bytes([FILL]) * 8
    # the text cut off in front of an unfinished header, as the pass over a file does
    if rec.unfinished >= 0:
        rows = _whole_records(rec._replace(gt_rank=rec.gt_rank[:-1], seq_rank=rec.seq_rank[:-1]),
                              int(rec.gt_rank[-1]))
        _check_gather(text, d, ix, rec, rows, n_records=rec.n - 1, nbytes=rec.unfinished)


def _locate(rec, text: bytes, p: int):
    """(record ordinal, contig position) of the kept text byte p."""
    r = int(np.searchsorted(rec.gt_pos, p, side="right"))
    rank = sum(c in KEEP for c in text[:p])
    return r, rank - (int(rec.seq_rank[r - 1]) if r else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("head", [0, 9])
def test_gather_intervals_across_tiles_and_inside_one_piece(gpu_device, head):
    T = _tile()
    rng = np.random.default_rng(77)
    # one long record over all tiles, a short one in front of it
    text = b">short\nACGT\n>long one\n" + b"".join(bytes(rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), 60)) + b"\n"
                                                    for _ in range(4 * T // 61))
    d, ix, rec = _check_index(text, head)
    assert rec.n == 2
    # from the middle of tile 0 to the last kept byte of tile 2: three tiles
    first = next(p for p in range(T // 2 - head, len(text)) if text[p] in KEEP)
    last = next(p for p in range(3 * T - 1 - head, 0, -1) if text[p] in KEEP)
    (r0, s), (r1, e) = _locate(rec, text, first), _locate(rec, text, last)
    assert r0 == r1 == 2 and e - s > 2 * T * 60 // 61
    got = _check_gather(text, d, ix, rec, [(2, s, e + 1, 0)])
    want = bytes(c for c in text[first:last + 1] if c in KEEP).upper()
    assert got[:e + 1 - s] == want and got[e + 1 - s:] == bytes([FILL]) * 8
    # pairs of intervals nine bytes apart, at every shift against the 16-byte pieces; the short record too
    rows, off = [(1, 1, 3, 0)], 2
    for k in range(16):
        p = 3 * T + 61 * k + k + 1 - head   # (inside a line of 60 letters)
        r, a = _locate(rec, text, p)
        for lo, hi in ((a, a + 3), (a + 5, a + 9)):
            rows.append((r, lo, hi, off))
            off += hi - lo
    got = _check_gather(text, d, ix, rec, rows)
    assert got[:2] == b"CG" and FILL not in got[:off]
    # no interval: nothing is written
    assert _check_gather(text, d, ix, rec, []) == bytes([FILL]) * 8


@pytest.mark.gpu
def test_capacities_and_host_memory(gpu_device):
    import torch
    from genefuserust_amd import _lib
    from genefuserust_amd.ref_cut import lib, ref_gather_device, ref_index_device
    text = _case("gt_all_four", 0)
    want = model_index(text)
    d = _device(text, 3)
    # cap_records one too small: the overflow bit, the first cap records, and nothing past the capacity
    cap = want.n - 1
    L = lib()
    i64 = lambda n, v=-7: torch.full((n,), v, dtype=torch.int64, device="cuda")
    arrays = [i64(cap + 4) for _ in range(4)]
    name_off, names, totals = i64(cap + 5), torch.full((1 << 14,), FILL, dtype=torch.uint8, device="cuda"), i64(8)
    ws = torch.empty(int(L.gf_rc_workspace_bytes(len(text))), dtype=torch.uint8, device="cuda")
    tile_kept = i64(int(L.gf_rc_tiles(len(text))) + 1)
    rc = L.gf_rc_index_device(d.data_ptr(), len(text), cap, ws.data_ptr(), ws.numel(), *(a.data_ptr() for a in arrays),
                              name_off.data_ptr(), names.data_ptr(), names.numel(), tile_kept.data_ptr(),
                              totals.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    tot = totals.cpu().tolist()
    assert tot[0] == want.n and tot[1] == want.kept and tot[2] & 1
    for a, f in zip(arrays[:2], ("gt_pos", "gt_rank")):
        assert a[:cap].cpu().tolist() == getattr(want, f)[:cap].tolist(), f
    for a in arrays:
        assert a[cap:].cpu().tolist() == [-7] * 4
    assert name_off[cap + 1:].cpu().tolist() == [-7] * 4
    # the mirror says what the call needs
    with pytest.raises(_lib.GfError) as e:
        ref_index_device(d, cap).download()
    assert e.value.code == _lib.GF_ERR_CAPACITY and e.value.needed == (want.n, None)
    need = sum(len(x) for x in want.names)
    with pytest.raises(_lib.GfError) as e:
        ref_index_device(d, want.n, need - 1).download()
    assert e.value.code == _lib.GF_ERR_CAPACITY and e.value.needed == (want.n, need)
    assert ref_index_device(d, want.n, need).download().names == want.names
    # a workspace that is too small
    rc = L.gf_rc_index_device(d.data_ptr(), len(text), cap, ws.data_ptr(), 8, *(a.data_ptr() for a in arrays),
                              name_off.data_ptr(), names.data_ptr(), names.numel(), tile_kept.data_ptr(),
                              totals.data_ptr(), None)
    assert rc == _lib.GF_ERR_CAPACITY and b"workspace" in L.gf_rc_last_error()
    # host memory is refused: by the mirror, and by the library itself
    host = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(_lib.GfError) as e:
        ref_index_device(host)
    assert e.value.code == _lib.GF_ERR_NO_DEVICE
    ix = ref_index_device(d, want.n)
    with pytest.raises(_lib.GfError) as e:
        ref_gather_device(host, ix, 0, [(0, 0, 1, 0)], 1)
    assert e.value.code == _lib.GF_ERR_NO_DEVICE
    arr = np.zeros(64, dtype=np.uint8)
    rc = L.gf_rc_index_device(arr.ctypes.data, 64, cap, ws.data_ptr(), ws.numel(), *(a.data_ptr() for a in arrays),
                              name_off.data_ptr(), names.data_ptr(), names.numel(), tile_kept.data_ptr(),
                              totals.data_ptr(), None)
    assert rc == _lib.GF_ERR_NO_DEVICE and b"not device memory" in L.gf_rc_last_error()
    rc = L.gf_rc_gather_device(arr.ctypes.data, 64, None, None, 0, tile_kept.data_ptr(), 0, arrays[0].data_ptr(), 1,
                               names.data_ptr(), 1, None)
    assert rc == _lib.GF_ERR_NO_DEVICE
    dst = torch.zeros(64, dtype=torch.uint8)
    assert L.gf_rc_copy_from_host_device(arr.ctypes.data, dst.data_ptr(), 64, None) == _lib.GF_ERR_NO_DEVICE
    # and the copy itself
    src = np.arange(64, dtype=np.uint8)
    ddst = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert L.gf_rc_copy_from_host_device(src.ctypes.data, ddst.data_ptr(), 64, None) == 0
    torch.cuda.synchronize()
    assert ddst.cpu().numpy().tolist() == src.tolist()
