"""The texts the device deflate is tested on (include/gf_deflate.h), shared by the host and the GPU tests: seeded, so
that both sides see the same bytes.  ``texts()``: {name: 2 * 65280 + 1 bytes}; a case is a text cut to one of ``SIZES``
(the device call also gets ``DEVICE_SIZES``).

The first nine are texts as files have them, and reach none of the encoder's hard branches.  The last five are laid out
around what the hash table holds (2048 entries, the largest position per hash, read a round of 64 positions late) so
that they do: ``window_edge`` a match at distance exactly 32768 and a copy one byte too far, ``deep_literals``,
``deep_distances`` and ``deep_code_lengths`` a Huffman tree past the 15, 15 and 7 bits its code may have,
``every_symbol`` every match length (5 .. 258) and every distance symbol.  Both members of each are built the same
way.  tests/test_deflate_core.py::test_what_every_text_reaches asserts what each reaches; what none does: match lengths
3 and 4 (gf_df_min_len is at least 5), and a length symbol with 5 extra bits behind a 15-bit code (a literal/length
code that deep takes a member of literals; no bounded search was made past that).  The 15-bit distance code with 13
extra bits, the widest unit, is ``deep_distances``', not ``every_symbol``'s, whose distance code is 9 deep."""
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
    far), between random filler of 16 letters (so that the member is worth a dynamic block).  Kept as a text; it emits
    no match at all, the filler having overwritten the motif's table entries by then: ``window_edge`` is the edge's."""
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


def _both_members(member) -> bytes:
    """2 * 65280 + 1 bytes: ``member(k)`` gives the 65280 bytes of member k = 0, 1, both built the same way."""
    a, b = member(0), member(1)
    assert len(a) == len(b) == TEXT
    return a + b + a[:1]


WINDOW_EDGE_AT = (100, 301)     # where the two motifs first stand; their second copies are 32768 and 32769 bytes on


def window_edge_member(k: int, reverse_the_near_copy: bool = False) -> bytes:
    """The farthest match and the first one too far.  A filler of period 2 has two 4-byte hashes, so the table entries of
    the motifs' hashes are still theirs 32768 positions on (random filler of 16 letters overwrites all 2048 entries long
    before that).  A 64-byte random motif stands at 100 and at 100 + 32768: within reach, one match of distance 32768.
    Another stands at 301 and at 301 + 32769: one too far.  ``reverse_the_near_copy``: the control, the same bytes at
    100 + 32768 in reverse order: the same histogram of bytes and nothing to copy."""
    rng = np.random.default_rng(23 + k)
    t = bytearray((b"AB" * TEXT)[:TEXT])
    a, b = (bytes(rng.integers(0, 256, 64, dtype=np.uint8)) for _ in range(2))
    t[WINDOW_EDGE_AT[0]:WINDOW_EDGE_AT[0] + 64] = a
    t[WINDOW_EDGE_AT[0] + 32768:WINDOW_EDGE_AT[0] + 32768 + 64] = a[::-1] if reverse_the_near_copy else a
    for at in (WINDOW_EDGE_AT[1], WINDOW_EDGE_AT[1] + 32769):
        t[at:at + 64] = b
    return bytes(t)


def deep_literals_member(k: int) -> bytes:
    """A literal code far past 15 bits: 16 byte values nearly equally often, and 16 others 1, 2, 3, 5, ... 1597 times
    (Fibonacci's numbers from the end-of-block symbol's count of 1 on, no two equal) at random places.  No matches to
    speak of; the unrestricted code is 20 bits deep."""
    rng = np.random.default_rng(29 + k)
    t = rng.integers(97, 113, TEXT, dtype=np.uint8)
    counts, a, b = [], 1, 2
    while len(counts) < 16:
        counts.append(a)
        a, b = b, a + b
    places = rng.permutation(TEXT)[:sum(counts)]
    t[places] = np.repeat(np.arange(33, 49, dtype=np.uint8), counts)
    return t.tobytes()


def gf_hash(b4) -> int:
    """gf_df_hash (gf_df_core.h) of 4 bytes: the texts below are laid out around what the table holds."""
    v = b4[0] | b4[1] << 8 | b4[2] << 16 | b4[3] << 24
    return ((v * 2654435761) & 0xffffffff) >> 21


def hashes(t) -> np.ndarray:
    """gf_df_hash at every position of ``t`` that has 4 bytes."""
    a = np.frombuffer(bytes(t), dtype=np.uint8).astype(np.uint64)
    v = a[:-3] | a[1:-2] << np.uint64(8) | a[2:-1] << np.uint64(16) | a[3:] << np.uint64(24)
    return ((v * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(21)


# -- deep_distances: blocks of 12 bytes (the least a match at distance 32768 takes), each one of 40 "colours"; a block
# is one match, of its colour's last block, so the distances are the text's to choose.
_BLOCK, _SUFFIX, _COLOURS, _WARM = 12, 3, 120, 40


def _palette(rng, want):
    """``want`` blocks c0 c1 m0 .. m6 z0 z1 z2, z the same in all: every 4 bytes in or across blocks depend on one block
    alone, and no block's first 4 bytes share their hash with any other 4 bytes.  So the table's entry for a block's
    start is its colour's last block, however far back (the low hash diversity that keeps a far candidate alive)."""
    z = bytes(rng.integers(0, 256, _SUFFIX, dtype=np.uint8))
    starts, others, out, firsts = set(), set(), [], set(z)
    while len(out) < want:
        blk = bytes(rng.integers(0, 256, _BLOCK - _SUFFIX, dtype=np.uint8)) + z
        if blk[0] in firsts:
            continue
        ring = z + blk
        grams = [gf_hash(ring[k:k + 4]) for k in range(len(ring) - 3)]
        s, o = grams[_SUFFIX], set(grams[:_SUFFIX] + grams[_SUFFIX + 1:])
        if s in starts or s in others or s in o or (o & starts):
            continue
        starts.add(s)
        others |= o
        out.append(blk)
        firsts.add(blk[0])
    return out


def _gaps_of(sym):
    """The gaps in blocks whose distance in bytes has the distance symbol ``sym``."""
    lo, hi = bgzf_members.DIST_BASE[sym], (bgzf_members.DIST_BASE[sym + 1] - 1 if sym < 29 else 32768)
    return range(-(-lo // _BLOCK), hi // _BLOCK + 1)


def deep_distances_demand():
    """{distance symbol: matches}: symbols 29 down to 13 in counts each greater than the sum of all but the last before
    it (Fibonacci's 1, 1, 2, 3, 5, ... with 4 % to spare from 300 on, for the few blocks that come out otherwise): a
    Huffman tree that is one chain, 16 deep.  13056 matches a member would allow a chain of 18."""
    c = [1, 1]
    while len(c) < 17:
        need = sum(c[:-1]) + 1
        c.append(need if need < 300 else int(need * 1.04) + 1)
    return {29 - k: f for k, f in enumerate(c)}


DEEP_DISTANCES_SEEDS = (1, 8)      # found by trying 1 .. 39: 7 of them give depth 16, these two first


def deep_distances_member(k: int) -> bytes:
    """A distance code past 15 bits, and a code-length code past 7: 5440 blocks, each the colour of an earlier block
    that no block between has, at a gap drawn from ``deep_distances_demand`` (the rare far ones first, as soon as a
    block that far back is free), never the gap of the block before (the two would be one match)."""
    rng = np.random.default_rng(DEEP_DISTANCES_SEEDS[k])
    pal = _palette(rng, _COLOURS)
    colour, head, ncol, prev_g = [], {}, 0, 0       # head: the blocks that are their colour's last
    left = deep_distances_demand()
    for b in range(TEXT // _BLOCK):
        pick = None
        if b >= _WARM:
            order = [s for s in sorted(left, reverse=True) if left[s] > 0 and s >= 20]
            rest = [s for s in left if left[s] > 0]
            for _ in range(6):
                if not rest:
                    break
                x, acc = rng.random() * sum(left[s] for s in rest), 0
                for s in rest:
                    acc += left[s]
                    if x < acc:
                        break
                order.append(s)
                rest.remove(s)
            for s in order:
                c = [g for g in _gaps_of(s) if head.get(b - g) and g != prev_g]
                if c:
                    pick = int(c[int(rng.integers(len(c)))])
                    left[s] -= 1
                    break
        if pick is None and (b < _WARM or not any(head.get(b - g) for g in range(9, b))):
            colour.append(ncol)         # a new colour: 12 literals
            ncol += 1
            prev_g = 0
        else:
            if pick is None:            # the nearest free block from 9 back
                pick = next(g for g in range(9, b) if head.get(b - g))
                prev_g = 0
            else:
                prev_g = pick
            colour.append(colour[b - pick])
            del head[b - pick]
        head[b] = True
    return b"".join(pal[c] for c in colour)


# -- deep_code_lengths: how many literals have a code of each length
DEEP_CODE_LENGTHS = {4: 1, 5: 1, 6: 2, 7: 89, 8: 13, 9: 55, 10: 8, 11: 21, 12: 3, 13: 5, 14: 34}
assert sum(n << (14 - l) for l, n in DEEP_CODE_LENGTHS.items()) == 1 << 14           # a complete code


def deep_code_lengths_member(k: int) -> bytes:
    """A code-length code past 7 bits: 231 byte values 2^(16 - length) times each, so that their code lengths are forced,
    the lengths 4 .. 14 taken by 1, 1, 2, 3, 5, ... 89 symbols (Fibonacci's numbers, put on the lengths so that the code
    is complete; the end-of-block symbol is one of the 34 of length 14) — the histogram of the lengths is one chain
    again, 9 deep with the 26 unused literals.  In random order: no value is frequent enough for 5-byte repeats."""
    rng = np.random.default_rng(31 + k)
    counts = [1 << (16 - l) for l, n in sorted(DEEP_CODE_LENGTHS.items()) for _ in range(n)][:-1]
    over, at = sum(counts) - TEXT, 0
    while over > 0:                      # 65280 is no power of two: the most frequent eight give the difference
        counts[at % 8] -= 1
        over -= 1
        at += 1
    return rng.permutation(np.repeat(np.arange(len(counts), dtype=np.uint8), counts)).tobytes()


# -- every_symbol
def every_symbol_member(k: int) -> bytes:
    """Every match length the encoder takes (5 .. 258: gf_df_min_len is 5 at the least) and every distance symbol
    (0 .. 29).  A filler of period 2 (two hashes); for the distance symbols 1 .. 11 a random stretch of that period
    from 12 .. 64 bytes before a round's first position on (the candidate lies in an earlier round); for 12 .. 29 twelve
    random bytes twice, the middle of the symbol's range apart, their hash met nowhere between; then a run of
    each length 6 .. 259 of a byte value of its own: a literal and a match of distance 1."""
    rng = np.random.default_rng(37 + k)
    runs = b"".join(bytes([v]) * (n + 1) for v, n in zip(rng.permutation(254).tolist(), range(5, 259)))
    free = TEXT - len(runs) - 1
    t = bytearray((b"\xfe\xff" * TEXT)[:free] + b"\xfe" + runs)
    taken = np.zeros(TEXT, dtype=bool)
    taken[free:] = True

    def plant(src, dst, n):
        """``n`` random bytes of period dst - src from ``src`` to ``dst + 12``, whose first four hash like no four bytes
        from ``src`` + 1 to ``dst``."""
        assert not (taken[src:dst + n].any() if dst - src < 12 else taken[src:src + 12].any() or taken[dst:dst + 12].any())
        while True:
            w = bytes(rng.integers(0, 254, min(dst - src, 12), dtype=np.uint8))
            if len(set(w[:4])) < min(4, len(w)):
                continue
            u = t[:]
            if dst - src < 12:
                u[src:dst + 12] = (w * 16)[:dst + 12 - src]
            else:
                u[src:src + 12] = u[dst:dst + 12] = w
            h = hashes(u)
            if not (h[src + 1:dst] == h[dst]).any():
                t[:] = u
                taken[src:src + 12] = taken[dst:dst + 12] = True
                if dst - src < 12:
                    taken[src:dst + 12] = True
                return
    at = 256
    for sym in range(1, 12):             # a stretch per symbol, its target a round's first position
        d = bgzf_members.DIST_BASE[sym] + (bgzf_members.DIST_EXTRA[sym] > 0)
        plant(at - d, at, 12)
        at += 128
    src = 2048
    for sym in range(12, 30):
        d = bgzf_members.DIST_BASE[sym] + (1 << bgzf_members.DIST_EXTRA[sym]) // 2     # the middle of its range
        while taken[src - 4:src + 16].any() or taken[src + d - 4:src + d + 16].any():
            src += 20
        plant(src, src + d, 12)
    assert len(t) == TEXT
    return bytes(t)


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
            "window_edge": _both_members(window_edge_member),
            "deep_literals": _both_members(deep_literals_member),
            "deep_distances": _both_members(deep_distances_member),
            "deep_code_lengths": _both_members(deep_code_lengths_member),
            "every_symbol": _both_members(every_symbol_member),
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
