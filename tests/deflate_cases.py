"""The texts the device deflate is tested on (include/gf_deflate.h), shared by the host and the GPU tests: seeded, so
that both sides see the same bytes.  ``texts()``: {name: 2 * 65280 + 1 bytes}; a case is a text cut to one of ``SIZES``
(the device call also gets ``DEVICE_SIZES``)."""
import struct
import zlib

import numpy as np

from tests import bgzf_members

TEXT = 65280
SIZES = (1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 257, 258, 259, 4096, 65279, 65280)
DEVICE_SIZES = SIZES + (65281, 2 * TEXT, 2 * TEXT + 1)
FULL = 2 * TEXT + 1
STORED_OVER = 31
STORED, DYNAMIC = 1, 2


def binned_fastq_text(nbytes: int, seed: int = 5) -> bytes:
    """FASTQ-like text whose qualities take four values, in runs (what current sequencers write)."""
    rng = np.random.default_rng(seed)
    out, n, i = [], 0, 0
    bins = np.frombuffer(b"#-<F", dtype=np.uint8)
    while n < nbytes:
        seq = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 150))
        qual = bytearray()
        while len(qual) < 150:
            qual += bytes([int(bins[rng.choice(4, p=(0.02, 0.08, 0.2, 0.7))])]) * int(rng.integers(1, 40))
        rec = b"@A00:77:HXXXX:%d:%d:%d:%d 1:N:0:ACGT\n%s\n+\n%s\n" % (1 + i % 4, 1101 + i // 50, 1000 + 7 * i, 2000 + i,
                                                                   seq, bytes(qual[:150]))
        out.append(rec)
        n += len(rec)
        i += 1
    return b"".join(out)[:nbytes]


def _motif(nbytes: int) -> bytes:
    """A 64-byte motif that recurs at distance exactly 32768 (the farthest a match may reach) and at 32769 (one too
    far), between random filler of 16 letters (so that the member is worth a dynamic block)."""
    rng = np.random.default_rng(11)
    t = bytearray(rng.integers(97, 113, nbytes, dtype=np.uint8).tobytes())
    a, b = bytes(rng.integers(0, 256, 64, dtype=np.uint8)), bytes(rng.integers(0, 256, 64, dtype=np.uint8))
    for at in (100, 100 + 32768):
        t[at:at + 64] = a
    for at in (300, 300 + 32769):
        t[at:at + 64] = b
    for at in (TEXT + 1000, TEXT + 1000 + 32768):     # the same in the second member
        t[at:at + 64] = a
    return bytes(t)


def _chained(nbytes: int) -> bytes:
    """Runs that force chained matches of length 258: 5000 bytes of one value, then a 700-byte random block three times
    over, then text."""
    rng = np.random.default_rng(13)
    block = bytes(rng.integers(0, 256, 700, dtype=np.uint8))
    t = b"Q" * 5000 + block * 3 + b"x" * 259 + block
    return (t * (nbytes // len(t) + 1))[:nbytes]


_cache = {}


def texts() -> dict:
    if not _cache:
        rng = np.random.default_rng(17)
        _cache.update({
            "fastq": bgzf_members.fastq_text(FULL, 3),
            "binned": binned_fastq_text(FULL),
            "one_byte_value": b"A" * FULL,
            "period_2": (b"AB" * FULL)[:FULL],
            "period_3": (b"xyz" * FULL)[:FULL],
            "all_values": (bytes(range(256)) * (FULL // 256 + 1))[:FULL],
            "random": rng.integers(0, 256, FULL, dtype=np.uint8).tobytes(),
            "motif_32768": _motif(FULL),
            "chained_258": _chained(FULL),
        })
    return _cache


def cases(sizes=SIZES):
    """[(name, size, text)]; the single byte is text size 1 of every text."""
    return [(name, size, t[:size]) for name, t in texts().items() for size in sizes]


def check_member(member: bytes, text: bytes) -> int:
    """``member`` is one BGZF member of ``text`` by every independent reading; returns its block kind (BTYPE)."""
    rows, used, total, why, _ = bgzf_members.walk_model(member)
    assert why == bgzf_members.WALK_END and used == len(member) and len(rows) == 1 and total == len(text)
    assert member[:16] == bytes.fromhex("1f8b08040000000000ff0600") + b"BC\x02\x00"
    assert struct.unpack_from("<H", member, 16)[0] == len(member) - 1                      # BSIZE
    assert struct.unpack("<II", member[-8:]) == (zlib.crc32(text), len(text))              # CRC-32, ISIZE
    assert zlib.decompress(member, 31) == text
    assert zlib.decompress(member[18:-8], -15) == text
    assert len(member) <= len(text) + STORED_OVER
    kind, final = bgzf_members.block_kinds(member[18:-8])
    assert final == 1 and kind in (0, 2)
    return kind
