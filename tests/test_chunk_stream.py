"""The host half of the chunk loop (genefuserust_amd/chunk_stream.py) without a GPU: the staged read over short reads,
the lending path and a gunzipped file; the read-size rules; and the loader of the companion libraries."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

N = 1000
TEXT = bytes(np.random.default_rng(5).integers(33, 127, N, dtype=np.uint8))
CHUNKS = [1, 5, 500, 999, 1000, 1001]


class _Dribble:
    """A byte source that hands out at most ``piece`` bytes per ``readinto``."""

    def __init__(self, text: bytes, piece: int):
        self.text, self.piece, self.pos = text, piece, 0

    def readinto(self, mv) -> int:
        n = min(len(mv), self.piece, len(self.text) - self.pos)
        mv[:n] = self.text[self.pos:self.pos + n]
        self.pos += n
        return n


def _side(source, chunk_bytes):
    from genefuserust_amd.chunk_stream import Side
    if hasattr(source, "take"):
        return Side(source, chunk_bytes)
    return Side(source, chunk_bytes, views=[memoryview(bytearray(chunk_bytes)) for _ in range(2)])


def _stage(side, slot, chunk_bytes):
    ptr, n = side.stage(slot, chunk_bytes)
    assert side.chunk_len[slot] == n
    if n == 0:
        return b""
    return C.string_at(ptr, n) if side.lends else bytes(side.views[slot][:n])


def _drain(side, chunk_bytes):
    """[(chunk, eof after it)] up to the chunk that sets ``eof``, the slots alternating as in the loop."""
    out, slot = [], 0
    while True:
        out.append((_stage(side, slot, chunk_bytes), side.eof))
        assert len(out) <= N + 1
        if side.eof:
            return out
        slot ^= 1


def _check_chunks(side, text, chunk_bytes):
    chunks = _drain(side, chunk_bytes)
    assert b"".join(c for c, _ in chunks) == text
    # eof on exactly the chunk that holds the last byte: full chunks in front of it, and no empty chunk behind a text
    # that the chunk size divides
    assert [e for _, e in chunks] == [False] * (len(chunks) - 1) + [True]
    assert all(len(c) == chunk_bytes for c, _ in chunks[:-1])
    assert len(chunks) == max(1, -(-len(text) // chunk_bytes))
    assert len(chunks[-1][0]) > 0 or not text
    # after the end: nothing
    for slot in (0, 1):
        assert _stage(side, slot, chunk_bytes) == b"" and side.eof


@pytest.mark.parametrize("piece", [1, 7, 13])
@pytest.mark.parametrize("chunk_bytes", CHUNKS)
def test_staged_read_over_short_reads(chunk_bytes, piece):
    _check_chunks(_side(_Dribble(TEXT, piece), chunk_bytes), TEXT, chunk_bytes)


@pytest.mark.parametrize("chunk_bytes", CHUNKS)
def test_staged_read_of_a_lent_array_and_of_a_gunzipped_file(chunk_bytes, tmp_path):
    from genefuserust_amd.chunk_stream import ArraySource
    from genefuserust_amd.fastq import FastqReader
    _check_chunks(_side(ArraySource(np.frombuffer(TEXT, dtype=np.uint8).copy()), chunk_bytes), TEXT, chunk_bytes)
    gz = tmp_path / "two_members.fq.gz"
    gz.write_bytes(gzip.compress(TEXT[:333]) + gzip.compress(TEXT[333:]))
    with FastqReader(str(gz)).open_stream() as source:
        _check_chunks(_side(source, chunk_bytes), TEXT, chunk_bytes)


def test_staged_read_of_empty_sources(tmp_path):
    from genefuserust_amd.chunk_stream import ArraySource
    from genefuserust_amd.fastq import FastqReader
    gz = tmp_path / "empty.fq.gz"
    gz.write_bytes(gzip.compress(b""))
    with FastqReader(str(gz)).open_stream() as zipped:
        for source in (_Dribble(b"", 7), ArraySource(np.zeros(0, dtype=np.uint8)), zipped):
            side = _side(source, 64)
            assert _drain(side, 64) == [(b"", True)]
            assert _stage(side, 1, 64) == b""


def test_read_chunk_keeps_the_byte_read_ahead():
    from genefuserust_amd.chunk_stream import read_chunk
    src, view = _Dribble(b"abcdefg", 2), memoryview(bytearray(3))
    assert read_chunk(src, view, 3, b"") == (3, b"d", False) and bytes(view) == b"abc"
    assert read_chunk(src, view, 3, b"d") == (3, b"g", False) and bytes(view) == b"def"
    assert read_chunk(src, view, 3, b"g") == (1, b"", True) and bytes(view[:1]) == b"g"


@pytest.mark.parametrize("starved", [True, False])
def test_the_fastq_rule_fills_the_chunk_behind_the_carry(starved):
    from genefuserust_amd.chunk_stream import fill_read_sizes
    c = 4096
    # a carry shorter than a chunk: what fills the chunk, starved or not
    assert fill_read_sizes(c, [(0, starved)]) == [c]
    assert fill_read_sizes(c, [(c - 1, starved)]) == [1]
    # a carry of a chunk or more: a record longer than a chunk takes the next chunk whole, a side that is ahead waits
    assert fill_read_sizes(c, [(c, starved)]) == [c if starved else 1]
    assert fill_read_sizes(c, [(c + 1, starved)]) == [c if starved else 1]


def test_read_sizes_of_two_sides_and_of_the_reference():
    from genefuserust_amd.chunk_stream import fill_read_sizes, whole_read_sizes
    c = 1000
    assert fill_read_sizes(c, [(0, True), (300, False)]) == [1000, 700]     # R2 is ahead: fewer new bytes
    assert fill_read_sizes(c, [(1500, False), (20, True)]) == [1, 980]      # R1 a chunk and more ahead: it waits
    assert fill_read_sizes(c, [(1500, True), (1500, True)]) == [1000, 1000]
    for carry in (0, c - 1, c, c + 1):
        for starved in (True, False):
            assert whole_read_sizes(c, [(carry, starved)]) == [c]


def test_a_companion_library_that_has_not_been_built():
    from genefuserust_amd import _lib
    path = os.path.join(_lib._HERE, "libgfmadeup.so")
    lib, check = _lib.companion(path, "made-up scan", "gf_xx_last_error", {"gf_xx_scan": (C.c_int, [C.c_void_p])})
    for call in (lib, lambda: check(-1)):
        with pytest.raises(ImportError) as e:
            call()
        assert str(e.value) == (
            "libgfmadeup.so not found at %s — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). The made-up scan has no CPU fallback." % path)
    assert check(0) == 0 and check(3) == 3
