"""libgfpack.so on the device: gf_pk_pack_device over synthetic scans — random bytes with planted totals, no index and no
reads — against ``tests/pack_model.py``, the whole block byte for byte, with sentinels behind it."""
import numpy as np
import pytest

from tests.pack_model import OVER_HITS, OVER_NAMES, OVER_RETRY, make_scan, pack_model, piece_kinds, same_scans
from tests.test_scan_pack_abi import source_define

FILL = 0xA5          # what the block and the sentinels behind it hold before the call
SENTINEL_BYTES = 256
SIZES = (0, 1, 15, 16, 17, 4097)


def _on_device(scans, offsets):
    """(PairScans, HitNames, aligns for ``piece_kinds``): scan i's byte tensors ``offsets[i]`` bytes off the 16-byte
    grid, its name offsets 8 bytes off it for an odd ``offsets[i]`` (an int64 array cannot be further off).  One arena,
    one upload: the tensors are views of it, with 0xEE between them."""
    import torch
    from genefuserust_amd.hit_names import HitNames
    from genefuserust_amd.read_pair import PairScan
    places, at = [], 0
    for s, o in zip(scans, offsets):
        row = []
        for arr, shift in ((s.hits, o), (s.bases, o), (s.quals, o), (s.totals, 0), (s.names, o),
                           (s.name_off, 8 * (o % 2)), (s.name_totals, 0)):
            at = (at + 15) // 16 * 16 + shift
            row.append((at, arr))
            at += arr.nbytes
        places.append(row)
    host = np.full(at + 16, 0xEE, dtype=np.uint8)
    for row in places:
        for pos, arr in row:
            host[pos:pos + arr.nbytes] = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    arena = torch.from_numpy(host).cuda()
    assert arena.data_ptr() % 16 == 0
    ps, hn, aligns = [], [], []
    for s, o, row in zip(scans, offsets, places):
        hits, bases, quals, totals, names, off, name_totals = (arena[pos:pos + arr.nbytes] for pos, arr in row)
        ps.append(PairScan(hits.view(-1, 64), bases, quals, totals.view(torch.int64)))
        hn.append(HitNames(names, off.view(torch.int64), name_totals.view(torch.int64)))
        aligns.append({"records": o, "bases": o, "quals": o, "names": (o + int(s.name_off[0])) % 16})
    return ps, hn, aligns


def _pack(ps, hn, block_bytes):
    """gf_pk_pack_device into a block of ``block_bytes`` with sentinels behind it: (the block's bytes, the sentinels)."""
    import torch
    from genefuserust_amd import _lib, scan_pack
    L = scan_pack.lib()
    k = len(ps)
    desc = torch.from_numpy(scan_pack.scan_descriptors(ps, hn).view(np.uint8)).cuda()
    ws_bytes = int(L.gf_pk_workspace_bytes(k))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    block = torch.full((block_bytes + SENTINEL_BYTES,), FILL, dtype=torch.uint8, device="cuda")
    scan_pack.check(L.gf_pk_pack_device(desc.data_ptr(), k, ws.data_ptr(), ws_bytes, block.data_ptr(), block_bytes,
                                        _lib.stream_handle(block.device)))
    torch.cuda.synchronize()
    host = block.cpu().numpy()
    return host[:block_bytes].tobytes(), host[block_bytes:].tobytes()


def _check(scans, offsets, spare=48):
    """The block of ``scans`` in a block with ``spare`` bytes of room: the model's bytes, nothing behind them."""
    ps, hn, aligns = _on_device(scans, offsets)
    want = pack_model(scans)
    got, sentinels = _pack(ps, hn, len(want) + spare)
    assert got[:64 * (len(scans) + 1)] == want[:64 * (len(scans) + 1)]            # the headers first: a clearer failure
    assert got[:len(want)] == want
    assert got[len(want):] == bytes([FILL]) * spare and sentinels == bytes([FILL]) * SENTINEL_BYTES
    return ps, hn, aligns, want


def _cycle(rng, k):
    """K scans: 0, 1, 2 records in turn and a few hundred every 16th; read and name bytes through SIZES; zero-record
    scans between the others."""
    out = []
    for i in range(k):
        rec = 300 + i % 7 if i % 16 == 5 else i % 3
        out.append(make_scan(rng, rec, SIZES[i % 6], SIZES[(i // 2 + 1) % 6] if rec else 0))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("offset", range(16))
def test_few_scans_at_every_source_offset(gpu_device, offset):
    """K = 1, 2, 3, every source ``offset`` bytes off the 16-byte grid; every count of records and every byte total."""
    rng = np.random.default_rng(100 + offset)
    for k in (1, 2, 3):
        for rec in (0, 1, 2, 257):
            scans = []
            for i in range(k):
                r = (rec + i) % 3 if rec < 3 else rec
                scans.append(make_scan(rng, r, SIZES[(offset + i + rec) % 6],
                                       SIZES[(offset + 2 * i + rec + 1) % 6] if r else 0))
            _check(scans, [offset] * k)
    # all the sizes at once, this offset
    _check([make_scan(rng, 2, b, n) for b, n in zip(SIZES, SIZES[::-1])], [offset] * 6)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [64, 65, 1024])
def test_many_scans(gpu_device, k):
    """K = 64, 65 (the plan's scan enters the block's second wavefront) and 1024; scan i is i mod 16 bytes off the
    grid, so that co-aligned, bytewise and straddling pieces all occur — counted in the model."""
    from genefuserust_amd.scan_pack import unpack_block
    scans = _cycle(np.random.default_rng(k), k)
    ps, hn, aligns, want = _check(scans, [i % 16 for i in range(k)])
    kinds = piece_kinds(scans, aligns)
    assert all(kinds[x] > 0 for x in ("aligned", "bytewise", "straddle", "offsets")), kinds
    same_scans(unpack_block(want, k), scans)


@pytest.mark.gpu
def test_overflowed_scans_are_packed_as_empty_between_their_neighbours(gpu_device):
    rng = np.random.default_rng(21)
    scans = [make_scan(rng, 2, 33, 20), make_scan(rng, 4, 50, 9, over=OVER_RETRY), make_scan(rng, 5, 160, 7),
             make_scan(rng, 4, 50, 9, over=OVER_HITS), make_scan(rng, 1, 1, 1), make_scan(rng, 4, 50, 9, names_over=True),
             make_scan(rng, 3, 16, 16), make_scan(rng, 4, 50, 9, over=OVER_RETRY | OVER_HITS, names_over=True),
             make_scan(rng, 300, 4097, 4097)]
    from genefuserust_amd.scan_pack import unpack_block
    _, _, _, want = _check(scans, [(3 * i + 1) % 16 for i in range(len(scans))])
    got = unpack_block(want, len(scans))
    assert [u.bits for u in got] == [0, OVER_RETRY, 0, OVER_HITS, 0, OVER_NAMES, 0, 7, 0]
    same_scans(got, scans)
    for i in (1, 3, 5, 7):
        assert len(got[i].rec) == 0 and got[i].bases == b"" and got[i].names == []
        assert got[i].totals["hits"] == int(scans[i].totals[0]) and got[i].name_bytes == int(scans[i].name_totals[1])


@pytest.mark.gpu
def test_block_exactly_as_needed_and_one_byte_less(gpu_device):
    rng = np.random.default_rng(31)
    scans = [make_scan(rng, 3, 17, 15), make_scan(rng, 0, 0, 0), make_scan(rng, 257, 4097, 16)]
    ps, hn, _, want = _check(scans, [5, 0, 11], spare=0)
    # one byte less: the headers are valid and say so; the body and what lies behind the block are untouched
    hb = 64 * (len(scans) + 1)
    got, sentinels = _pack(ps, hn, len(want) - 1)
    assert got[:hb] == pack_model(scans, block_bytes=len(want) - 1)
    head = np.frombuffer(got[:hb], dtype="<i8").reshape(-1, 8)
    assert head[0, 0] == len(want) - hb and head[0, 2] == 1 and (head[1:, 0] == [3, 0, 257]).all()
    assert got[hb:] == bytes([FILL]) * (len(want) - 1 - hb) and sentinels == bytes([FILL]) * SENTINEL_BYTES
    # the headers alone
    got, sentinels = _pack(ps, hn, hb)
    assert got == pack_model(scans, block_bytes=hb) and sentinels == bytes([FILL]) * SENTINEL_BYTES


@pytest.mark.gpu
def test_one_piece_more_than_a_full_pass_of_the_copy_grid(gpu_device):
    """The copy kernel's grid is capped and strides: a body of GF_PK_COPY_BLOCKS * 256 pieces and one more."""
    pass_pieces = source_define("GF_PK_COPY_BLOCKS") * 256
    assert source_define("GF_PK_PIECE") == 16
    # bases and qualities of pass_pieces / 2 pieces each, and the one name offset of a scan without records
    scans = [make_scan(np.random.default_rng(41), 0, pass_pieces // 2 * 16, 0)]
    _, _, _, want = _check(scans, [0])
    assert len(want) - 64 * 2 == (pass_pieces + 1) * 16


@pytest.mark.gpu
def test_pack_scans_device_and_download(gpu_device, monkeypatch):
    """The Python half: two copies; a block that is too small is packed again from its header's size."""
    from genefuserust_amd import scan_pack
    rng = np.random.default_rng(51)
    scans = _cycle(rng, 20) + [make_scan(rng, 4, 50, 9, over=OVER_HITS)]
    ps, hn, _ = _on_device(scans, [i % 16 for i in range(len(scans))])
    copies = []
    to_host = scan_pack._to_host
    monkeypatch.setattr(scan_pack, "_to_host", lambda t: (copies.append(t.numel()), to_host(t))[1])
    want = pack_model(scans)
    same_scans(scan_pack.pack_scans_device(ps, hn).download(), scans)
    assert copies == [64 * 22, len(want) - 64 * 22]            # the headers, then exactly the body
    del copies[:]
    same_scans(scan_pack.pack_scans_device(ps, hn, block_bytes=len(want) - 1).download(), scans)
    assert copies == [64 * 22, 64 * 22, len(want) - 64 * 22]
    # a scan without anything: one copy would do, and a second one of nothing is not made
    del copies[:]
    empty = [make_scan(rng, 4, 50, 9, over=OVER_RETRY)]
    e_ps, e_hn, _ = _on_device(empty, [7])
    same_scans(scan_pack.pack_scans_device(e_ps, e_hn).download(), empty)
    assert copies == [128]
