"""``bgzf.BgzfSource`` without a GPU, the inflate call replaced by zlib: the pieces a side hands out, ``final`` and the
straddling remainder are those of ``read_chunk`` over the plain text, for any chunk size."""
import gzip
import zlib

import pytest

from tests import bgzf_members as bm

TEXT = bm.fastq_text(300000, seed=6)
SIZES = (65280, 4000, 1)
CHUNKS = [1, 4096, 65279, 65280, 65281, 1 << 20]


def _host_pieces(text: bytes, chunk_bytes: int, limit: int):
    """[(piece, final)] of the host route: ``Side.stage`` over the plain text."""
    from genefuserust_amd.chunk_stream import Side

    class Plain:
        def __init__(self):
            self.pos = 0

        def readinto(self, mv):
            n = min(len(mv), len(text) - self.pos)
            mv[:n] = text[self.pos:self.pos + n]
            self.pos += n
            return n
    side = Side(Plain(), chunk_bytes, views=[memoryview(bytearray(chunk_bytes)) for _ in range(2)])
    out, slot = [], 0
    while len(out) < limit:
        _, n = side.stage(slot, chunk_bytes)
        out.append((bytes(side.views[slot][:n]), side.eof))
        if side.eof:
            break
        slot ^= 1
    return out


def _device_pieces(path, chunk_bytes: int, limit: int, sizes=None):
    """The same from a ``BgzfSource``: the staged members inflated by zlib, the chunk put together by
    ``bgzf.assemble``.  ``sizes``: the read size per call (default: ``chunk_bytes`` every time)."""
    from genefuserust_amd import bgzf
    from genefuserust_amd.chunk_stream import Side
    with bgzf.BgzfSource(str(path)) as source:
        block = source.staging_bytes(chunk_bytes)
        side = Side(source, chunk_bytes, views=[memoryview(bytearray(block)) for _ in range(2)])
        assert side.inflates and not side.lends
        out, slot, remainder = [], 0, b""
        while len(out) < limit:
            nbytes = chunk_bytes if sizes is None else sizes[len(out) % len(sizes)]
            ptr, n = side.stage(slot, nbytes)
            c = side.chunks[slot]
            assert ptr is None and n == c.comp_len and side.chunk_len[slot] == c.text_len
            comp = bytes(side.views[slot][:n])
            # whole members, back to back, exactly the staged bytes
            w = bgzf.walk_blocks(comp)
            assert w.why == bgzf.WALK_END and w.table[:, :5].tolist() == c.table[:, :5].tolist() and w.comp_bytes == n
            new = b"".join(zlib.decompress(comp[r[0]:r[0] + r[1]], -15) for r in c.table)
            text, remainder = bgzf.assemble(c, remainder, new)
            assert len(remainder) < bm.MAX_TEXT and len(text) == min(nbytes, len(text) + len(remainder)) or side.eof
            out.append((text, side.eof))
            if side.eof:
                assert remainder == b""
                assert side.stage(slot ^ 1, nbytes) == (None, 0) and side.chunks[slot ^ 1] is None
                break
            slot ^= 1
        return out


@pytest.fixture(scope="module")
def bgzf_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("bgzf") / "reads.fq.gz"
    p.write_bytes(bm.bgzf(TEXT, SIZES))
    assert gzip.decompress(p.read_bytes()) == TEXT
    return p


@pytest.mark.parametrize("chunk_bytes", CHUNKS)
def test_pieces_are_the_host_routes(bgzf_file, chunk_bytes):
    limit = 70000 if chunk_bytes == 1 else 1 << 30     # (one-byte chunks: across the first member's end, not the file)
    assert _device_pieces(bgzf_file, chunk_bytes, limit) == _host_pieces(TEXT, chunk_bytes, limit)


def test_read_sizes_that_change(bgzf_file):
    """The FASTQ rule asks for another size every time, one byte among them."""
    sizes = [5000, 1, 65280, 1, 1, 70000, 3]
    got = _device_pieces(bgzf_file, 70000, 1 << 30, sizes)
    pos = 0
    for k, (piece, final) in enumerate(got):
        assert piece == TEXT[pos:pos + sizes[k % len(sizes)]]
        pos += len(piece)
        assert final == (pos == len(TEXT))
    assert pos == len(TEXT)


@pytest.mark.parametrize("shape", ["no_marker", "markers_everywhere", "exact_end", "only_marker", "one_byte"])
def test_ends_of_files(tmp_path, shape):
    m = bm.member
    text = TEXT[:10000]
    members = {"no_marker": [m(text[:6000]), m(text[6000:])],
               "markers_everywhere": [bm.EOF_MARKER, m(text[:6000]), bm.EOF_MARKER, bm.EOF_MARKER, m(text[6000:]),
                                      bm.EOF_MARKER, bm.EOF_MARKER],
               "exact_end": [m(text[:5000]), m(text[5000:]), bm.EOF_MARKER],
               "only_marker": [bm.EOF_MARKER], "one_byte": [m(text[:1]), bm.EOF_MARKER]}[shape]
    p = tmp_path / "f.gz"
    p.write_bytes(b"".join(members))
    plain = gzip.decompress(p.read_bytes())
    for chunk_bytes in (1, 5000, 6000, 10000, 10001):
        assert _device_pieces(p, chunk_bytes, 1 << 30) == _host_pieces(plain, chunk_bytes, 1 << 30), chunk_bytes


def test_what_is_not_bgzf_and_what_is_cut(tmp_path):
    m = bm.member
    text = TEXT[:10000]
    p = tmp_path / "second_is_gzip.gz"
    p.write_bytes(m(text[:6000]) + gzip.compress(text[6000:]))
    # the chunk that ends inside the first member is had; the next one is not
    assert _device_pieces(p, 5000, 1) == [(text[:5000], False)]
    for chunk_bytes in (5000, 6000, 10000):
        with pytest.raises(ValueError) as e:
            _device_pieces(p, chunk_bytes, 1 << 30)
        assert "offset %d" % len(m(text[:6000])) in str(e.value) and 'inflate="host"' in str(e.value)
    whole = m(text[:6000]) + m(text[6000:])
    for cut in (len(whole) - 1, len(m(text[:6000])) + 5, len(m(text[:6000])) - 3):
        p = tmp_path / ("cut_%d.gz" % cut)
        p.write_bytes(whole[:cut])
        for chunk_bytes in (5000, 6000, 10000):
            with pytest.raises(EOFError):
                _device_pieces(p, chunk_bytes, 1 << 30)
            with pytest.raises(EOFError):
                gzip.decompress(whole[:cut])


def test_members_too_small_for_the_staging_block(tmp_path):
    from genefuserust_amd import _lib
    p = tmp_path / "tiny_members.gz"
    p.write_bytes(bm.bgzf(TEXT[:60000], (1,)))     # 29 bytes a byte of text
    with pytest.raises(_lib.GfError) as e:
        _device_pieces(p, 1 << 20, 1 << 30)
    assert e.value.code == _lib.GF_ERR_CAPACITY


def test_which_files_go_to_the_device(tmp_path, bgzf_file):
    from genefuserust_amd import bgzf
    plain, gz, empty = tmp_path / "a.fq", tmp_path / "a.fq.gz", tmp_path / "e.fq.gz"
    plain.write_bytes(TEXT[:100])
    gz.write_bytes(gzip.compress(TEXT[:100]))
    empty.write_bytes(b"")
    assert bgzf.is_bgzf(str(bgzf_file)) and not bgzf.is_bgzf(str(gz)) and not bgzf.is_bgzf(str(empty))
    for mode, want in (("host", [False] * 4), ("auto", [True, False, False, False])):
        assert [bgzf.use_device_inflate(str(f), mode) for f in (bgzf_file, gz, plain, empty)] == want
    assert bgzf.use_device_inflate(str(bgzf_file), "device") and not bgzf.use_device_inflate(str(plain), "device")
    with pytest.raises(ValueError) as e:
        bgzf.use_device_inflate(str(gz), "device")
    assert str(gz) in str(e.value)
    with pytest.raises(ValueError):
        bgzf.use_device_inflate(str(plain), "gpu")
    with pytest.raises(ValueError):
        bgzf.need_chunks("device", False, "chunk_bytes")
    bgzf.need_chunks("host", False, "chunk_bytes")
    bgzf.need_chunks("auto", True, "chunk_bytes")
