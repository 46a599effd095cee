"""libgfdeflate.so on the device (include/gf_deflate.h): ``gf_df_deflate_device`` against ``gf_df_member_host``, the host
statement of the same encoder (tests/test_deflate_core.py holds that one to zlib), byte for byte and member by member —
with every buffer inside junk that must stay, the text at every alignment and ending at its buffer's last byte, a true
length on the device below the capacity; the output inflated again on the device; and the streamed scans writing
``.gz`` files with ``ReadWriter(deflate="device")`` against the host route."""
import functools
import gzip
import os

import numpy as np
import pytest

from genefuserust_amd import deflate as df
from genefuserust_amd.read_write import ReadWriter
from tests import bgzf_members as bm
from tests import deflate_cases as dc
from tests.test_read_write_gpu import CHUNK, _all_steps, _read, _texts, files   # noqa: F401  (the routes' small fixtures)

pytestmark = pytest.mark.gpu
GUARD, JUNK = 64, 0xA5
T = dc.TEXT
NEW_TEXTS = ("window_edge", "deep_literals", "deep_distances", "deep_code_lengths", "every_symbol")


@functools.lru_cache(maxsize=None)
def host_member(text: bytes) -> bytes:
    return df.deflate_member_host(text)


def host_members(text: bytes):
    return [host_member(text[k:k + T]) for k in range(0, len(text), T)]


def device_deflate(text: bytes, true_len=None, lead: int = 0, out_lead: int = 0):
    """One raw ``gf_df_deflate_device`` call over ``text`` as the capacity, ``true_len`` (None: no pointer) as the length
    on the device: (output bytes, member offsets, totals added), after the checks that the text and the junk around the
    output, the offsets and the exact-size workspace stayed.  ``lead``: the alignment of the text's first byte; its
    last byte is its buffer's last."""
    import torch
    cap = len(text)
    members, out_cap = df.members(cap), df.out_cap(cap)
    L = df.lib()
    assert L.gf_df_members(cap) == members and L.gf_df_out_cap(cap) == out_cap
    whole = torch.from_numpy(np.frombuffer(bytes([JUNK]) * (GUARD + lead) + text, dtype=np.uint8).copy()).cuda()
    assert whole.data_ptr() % 16 == 0
    before = whole.clone()
    out = torch.full((GUARD + out_lead + out_cap + GUARD,), JUNK, dtype=torch.uint8, device="cuda")
    member_off = torch.full((members + 1 + 8,), -77, dtype=torch.int64, device="cuda")
    ws_bytes = int(L.gf_df_workspace_bytes(cap))
    ws = torch.full((ws_bytes + GUARD,), 0x3C, dtype=torch.uint8, device="cuda")
    start = [1000, 5, 0, 7, 70]
    totals = torch.tensor(start, dtype=torch.int64, device="cuda")
    length = None if true_len is None else torch.tensor([true_len], dtype=torch.int64, device="cuda")
    df.check(L.gf_df_deflate_device(whole.data_ptr() + GUARD + lead, cap, None if length is None else length.data_ptr(),
                                    out.data_ptr() + GUARD + out_lead, out_cap, member_off.data_ptr(), totals.data_ptr(),
                                    ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(whole, before)
    assert (ws.cpu().numpy()[ws_bytes:] == 0x3C).all()
    off = member_off.cpu().numpy()
    assert (off[members + 1:] == -77).all()
    total = int(off[members])
    assert 0 <= total <= out_cap
    o = out.cpu().numpy()
    first = GUARD + out_lead
    assert (o[:first] == JUNK).all() and (o[first + total:] == JUNK).all()       # nothing outside the members
    return o[first:first + total].tobytes(), [int(x) for x in off[:members + 1]], \
        [a - b for a, b in zip(totals.cpu().tolist(), start)]


def against_the_host(text: bytes, true_len=None, lead: int = 0, out_lead: int = 0):
    live = text if true_len is None else text[:max(0, min(true_len, len(text)))]
    want = host_members(live)
    got, off, totals = device_deflate(text, true_len, lead, out_lead)
    starts = np.concatenate([[0], np.cumsum([len(m) for m in want])]).astype(int).tolist()
    absent = df.members(len(text)) - len(want)
    for k, m in enumerate(want):
        assert got[starts[k]:starts[k + 1]] == m, ("member", k)
    assert got == b"".join(want)
    assert off == starts + [starts[-1]] * absent          # an absent member starts where the output ends
    stored = sum(1 for m in want if bm.block_kinds(m[18:-8])[0] == 0)
    assert totals == [len(want), len(live), len(got), stored, len(want) - stored]
    return got


def test_every_text_at_every_size_is_the_host_models_bytes(gpu_device):
    stored = dynamic = 0
    for k, (name, size, text) in enumerate(dc.cases(dc.DEVICE_SIZES)):
        got = against_the_host(text, lead=k % 16, out_lead=(5 * k) % 16)
        kinds = [bm.block_kinds(bytes(m[18:-8]))[0] for m in host_members(text)]
        stored, dynamic = stored + kinds.count(0), dynamic + kinds.count(2)
        if size in (65281, 2 * T + 1):      # the members walk, and gunzip to the text
            assert gzip.decompress(got + df.EOF_MARKER) == text, (name, size)
    assert stored > 50 and dynamic > 50


def test_every_alignment_of_the_text_and_the_output(gpu_device):
    texts = dc.texts()
    for lead in range(16):
        against_the_host(texts["fastq"][:T + 4096 + lead], lead=lead, out_lead=15 - lead)
        against_the_host(texts["binned"][:4096 - lead], lead=lead, out_lead=lead)


def test_the_true_length_is_read_on_the_device(gpu_device):
    """``d_text_bytes`` below the capacity: the members past it write nothing and count as absent; 0 gives none."""
    text = dc.texts()["binned"]
    for true_len in (0, 1, 4096, T - 1, T, T + 1, 2 * T, 2 * T + 1):
        against_the_host(text, true_len, lead=true_len % 16)
    got, off, totals = device_deflate(text, 0)
    assert got == b"" and off == [0, 0, 0, 0] and totals == [0] * 5
    # out of range on either side is cut to the capacity's range
    assert against_the_host(text[:5000], 1 << 40) == against_the_host(text[:5000])
    assert against_the_host(text[:5000], -3) == b""


def test_two_runs_give_the_same_bytes(gpu_device):
    for name in ("fastq", "chained_258", "motif_32768") + NEW_TEXTS:
        text = dc.texts()[name]
        assert device_deflate(text, lead=3) == device_deflate(text, lead=3)


def test_the_binding_and_the_device_inflate_read_it_back(gpu_device):
    """``deflate_device`` over a tensor, its length a device tensor; ``gf_if_walk_blocks`` and ``gf_if_inflate_device``
    over the output: every member status 0, and the text is back."""
    import torch
    from genefuserust_amd import bgzf
    for name, text in dc.texts().items():
        d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
        true_len = len(text) - 77
        out, member_off, totals = df.deflate_device(d_text, torch.tensor([true_len], dtype=torch.int64, device="cuda"))
        t = totals.cpu().tolist()
        n = df.members(true_len)
        assert n == 2 and member_off.numel() == 4           # the third member is absent
        assert t[:2] == [n, true_len] and t[2] == int(member_off[-1]) and out.numel() == df.out_cap(len(text))
        comp = out[:t[2]].cpu().numpy()
        assert comp.tobytes() == b"".join(host_members(text[:true_len])), name
        walk = bgzf.walk_blocks(comp)
        assert (walk.members, walk.comp_bytes, walk.text_bytes, walk.why) == (n, t[2], true_len, bm.WALK_END)
        assert walk.table[:, 0].tolist() == [int(x) + 18 for x in member_off[:n].cpu().tolist()]
        back = torch.full((true_len + 16,), JUNK, dtype=torch.uint8, device="cuda")
        status, totals = bgzf.inflate_device(out[:t[2]], torch.from_numpy(walk.table.copy()).cuda(), back)
        assert status.cpu().tolist() == [0] * n and totals.cpu().tolist() == [n, -1, 0, true_len], name
        assert back[:true_len].cpu().numpy().tobytes() == text[:true_len] and set(back[true_len:].cpu().tolist()) == {JUNK}
    out, member_off, totals = df.deflate_device(torch.empty(0, dtype=torch.uint8, device="cuda"))
    assert member_off.cpu().tolist() == [0] and totals.cpu().tolist() == [0] * 5


def test_the_texts_at_the_limits_come_back_through_the_device_inflate(gpu_device):
    """The texts made for the code-length limits and the window's edge (tests/test_deflate_core.py pins what each
    reaches), whole: three members each from the device deflate, the host model's bytes, and the device inflate gives
    the text back, every status 0."""
    import torch
    from genefuserust_amd import bgzf
    for name in NEW_TEXTS:
        text = dc.texts()[name]
        out, member_off, totals = df.deflate_device(torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda())
        t = totals.cpu().tolist()
        assert t[:2] == [3, len(text)] and t[3:] == [1, 2], name          # two dynamic members and the single byte, stored
        comp = out[:t[2]].cpu().numpy()
        assert comp.tobytes() == b"".join(host_members(text)), name
        walk = bgzf.walk_blocks(comp)
        assert (walk.members, walk.comp_bytes, walk.text_bytes, walk.why) == (3, t[2], len(text), bm.WALK_END)
        back = torch.full((len(text) + 16,), JUNK, dtype=torch.uint8, device="cuda")
        status, totals = bgzf.inflate_device(out[:t[2]], torch.from_numpy(walk.table.copy()).cuda(), back)
        assert status.cpu().tolist() == [0] * 3 and totals.cpu().tolist() == [3, -1, 0, len(text)], name
        assert back[:len(text)].cpu().numpy().tobytes() == text and set(back[len(text):].cpu().tolist()) == {JUNK}, name


def test_host_memory_is_refused(gpu_device):
    import torch
    from genefuserust_amd import _lib
    L = df.lib()
    cap = 1000
    good = dict(text=torch.zeros(cap, dtype=torch.uint8, device="cuda"), length=torch.tensor([cap], device="cuda"),
                out=torch.zeros(df.out_cap(cap), dtype=torch.uint8, device="cuda"),
                off=torch.zeros(2, dtype=torch.int64, device="cuda"), totals=torch.zeros(5, dtype=torch.int64, device="cuda"),
                ws=torch.zeros(int(L.gf_df_workspace_bytes(cap)), dtype=torch.uint8, device="cuda"))
    host = torch.zeros(int(L.gf_df_workspace_bytes(cap)) // 8 + 8, dtype=torch.int64)
    for bad in good:
        p = {k: (host if k == bad else t).data_ptr() for k, t in good.items()}
        rc = L.gf_df_deflate_device(p["text"], cap, p["length"], p["out"], df.out_cap(cap), p["off"], p["totals"], p["ws"],
                                    good["ws"].numel(), None)
        assert rc == _lib.GF_ERR_NO_DEVICE and b"no CPU fallback" in L.gf_df_last_error(), bad
    torch.cuda.synchronize()
    assert good["totals"].cpu().tolist() == [0] * 5


# ---- the streamed routes ----------------------------------------------------------------------------------------------------

def _markers(path):
    """(members, members of no text, whether the file ends with the marker) of a BGZF file."""
    data = _read(path)
    rows, used, _, why, _ = bm.walk_model(data)
    assert why == bm.WALK_END and used == len(data)
    return len(rows), sum(1 for r in rows if r[3] == 0), data.endswith(df.EOF_MARKER)


def test_pair_route_device_deflate_against_the_host_route(files, tmp_path):   # noqa: F811
    from genefuserust_amd.scan import scan_pair_end_report
    f = files
    args = (f["fa"], f["csvs"][3], f["w1"], f["w2"])
    got, outs = {}, {}
    for route in ("host", "device"):
        w = ReadWriter(str(tmp_path / (route + "_1.fq.gz")), str(tmp_path / (route + "_2.fq.gz")), umi_in_name=True,
                       deflate=route)
        got[route] = scan_pair_end_report(*args, chunk_bytes=CHUNK, **_all_steps(f), write_reads=w)
        outs[route] = w
    assert got["device"][1]["chunks"] >= 3
    assert got["device"][1] == got["host"][1] and list(got["device"][1]) == list(got["host"][1])     # every counter
    assert _texts(got["device"][0]) == _texts(got["host"][0]) and len(got["host"][0]) > 0           # every match
    want = f["want_pairs"]["tagged"]
    for side, (h, d) in enumerate(zip(outs["host"].outputs, outs["device"].outputs)):
        assert gzip.decompress(_read(d)) == gzip.decompress(_read(h)) == want.texts[side]
        members, empty, ends = _markers(d)
        assert members >= 4 and empty == 1 and ends          # three chunks and more, exactly one marker, at the end
        assert outs["device"].compressed_bytes[side] == os.path.getsize(d) - len(df.EOF_MARKER)
        assert not os.path.exists(d + ".tmp")
    assert outs["host"].compressed_bytes is None
    assert outs["device"].result() == outs["host"].result()      # written_*: text bytes, before compression
    assert outs["device"].result().bytes == tuple(want.totals[2:4])


def test_single_end_route_and_the_files_scanned_again_with_the_device_inflate(files, tmp_path):   # noqa: F811
    from genefuserust_amd.scan import scan_pair_end_files, scan_single_end_files
    f = files
    w = ReadWriter(str(tmp_path / "s.fq.gz"), deflate="device")
    h = ReadWriter(str(tmp_path / "h.fq.gz"))
    got = scan_single_end_files(f["fa"], f["csvs"][3], f["w1"], chunk_bytes=CHUNK, **_all_steps(f, single=True), write_reads=w)
    host = scan_single_end_files(f["fa"], f["csvs"][3], f["w1"], chunk_bytes=CHUNK, **_all_steps(f, single=True), write_reads=h)
    assert got == host and got[1]["chunks"] >= 3
    assert gzip.decompress(_read(w.out1)) == gzip.decompress(_read(h.out1)) == f["want_single"]["plain"].texts[0]
    assert _markers(w.out1)[1:] == (1, True)
    # a scan that writes no record leaves just the marker: tested on the host in test_deflate_plumbing.py
    # the pair files, written plain and by the device deflate, scanned again: the second strictly on the device inflate
    plain = ReadWriter(str(tmp_path / "p1.fq"), str(tmp_path / "p2.fq"))
    packed = ReadWriter(str(tmp_path / "d1.fq.gz"), str(tmp_path / "d2.fq.gz"), deflate="device")
    args = (f["fa"], f["csvs"][3], f["w1"], f["w2"])
    scan_pair_end_files(*args, chunk_bytes=CHUNK, **_all_steps(f), write_reads=plain)
    scan_pair_end_files(*args, chunk_bytes=CHUNK, **_all_steps(f), write_reads=packed)
    again_plain = scan_pair_end_files(f["fa"], f["csvs"][3], plain.out1, plain.out2, chunk_bytes=1 << 22)
    again = scan_pair_end_files(f["fa"], f["csvs"][3], packed.out1, packed.out2, chunk_bytes=1 << 22, inflate="device")
    assert [(m.m_name, m.m_read) for m in again[0]] == [(m.m_name, m.m_read) for m in again_plain[0]] and len(again[0]) > 0
    assert again[1] == again_plain[1] and again[1]["pairs"] == f["want_pairs"]["plain"].totals[0]
