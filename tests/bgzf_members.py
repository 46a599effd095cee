"""BGZF members for the tests of the device inflate: members made by zlib in every block kind, members assembled bit by
bit that zlib cannot emit but must accept, malformed members, and ``walk_model``, a restatement of gf_if_walk_blocks
(include/gf_inflate.h) in Python.  The expected text comes from zlib / gzip everywhere.  ``deep_codes``: members at the
limits of the code lengths; ``tokens_of``: a dynamic block taken apart into its code lengths and tokens."""
import struct
import zlib

import numpy as np

# the statuses of genefuserust_amd/scan_csrc/gf_if_core.h
(OK, BAD_BTYPE, STORED_LEN, BAD_COUNTS, OVERSUBSCRIBED, INCOMPLETE, REPEAT_FIRST, LENGTHS_OVERRUN, NO_END_CODE, BAD_LITLEN,
 BAD_DIST_SYM, DIST_TOO_FAR, OUTPUT_OVERRUN, OUTPUT_SHORT, INPUT_EXHAUSTED, CRC, BAD_ROW, BAD_CODE, TRAILING) = range(19)
# why a walk stopped
WALK_END, WALK_INSIDE, WALK_BUDGET, WALK_CAPACITY, WALK_NOT_BGZF = range(5)
ROW = 6
MAX_TEXT = 65536


def fastq_text(nbytes: int, seed: int = 1) -> bytes:
    """``nbytes`` of FASTQ-like text: 150-base records with names, '+' lines and qualities."""
    rng = np.random.default_rng(seed)
    out, n, i = [], 0, 0
    while n < nbytes:
        seq = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 150))
        qual = bytes(rng.integers(35, 74, 150, dtype=np.uint8))
        rec = b"@read%d/1 lane:%d\n%s\n+\n%s\n" % (i, seed, seq, qual)
        out.append(rec)
        n += len(rec)
        i += 1
    return b"".join(out)[:nbytes]


def raw_deflate(text: bytes, level: int = -1, strategy: int = zlib.Z_DEFAULT_STRATEGY) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(text) + c.flush()


def wrap(payload: bytes, crc: int, isize: int, extra_front: bytes = b"") -> bytes:
    """A BGZF member around a raw DEFLATE payload: the 18-byte header (longer by ``extra_front``, extra subfields put
    before ``BC``), CRC-32 and ISIZE."""
    xlen = len(extra_front) + 6
    bsize = 12 + xlen + len(payload) + 8
    assert bsize <= 65536
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra_front + b"BC\x02\0"
            + struct.pack("<H", bsize - 1) + payload + struct.pack("<II", crc & 0xffffffff, isize))


def member(text: bytes, level: int = -1, strategy: int = zlib.Z_DEFAULT_STRATEGY, extra_front: bytes = b"") -> bytes:
    return wrap(raw_deflate(text, level, strategy), zlib.crc32(text), len(text), extra_front)


EOF_MARKER = member(b"")
assert EOF_MARKER == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf(text: bytes, sizes=(65280,), level: int = 6, eof: bool = True) -> bytes:
    """``text`` as a BGZF file: members of ``sizes`` text bytes in turn, and the end-of-file marker."""
    out, pos, k = [], 0, 0
    while pos < len(text):
        n = sizes[k % len(sizes)]
        out.append(member(text[pos:pos + n], level))
        pos += n
        k += 1
    return b"".join(out) + (EOF_MARKER if eof else b"")


def block_kinds(payload: bytes):
    """(BTYPE of the first deflate block, whether it is final)."""
    return (payload[0] >> 1) & 3, payload[0] & 1


def kinds():
    """[(name, text, member)]: the block kinds zlib emits (the issue's table)."""
    fq = fastq_text(65280)
    rnd = bytes(np.random.default_rng(7).integers(0, 256, 65280, dtype=np.uint8))
    cases = [("stored_level0", fq[:60000], dict(level=0)), ("stored_random", rnd, {}),
             ("fixed", fq, dict(strategy=zlib.Z_FIXED)), ("one_byte", b"G", {}), ("empty", b"", {}),
             ("level1", fq, dict(level=1)), ("level6", fq, dict(level=6)), ("level9", fq, dict(level=9)),
             ("huffman_only", fq, dict(strategy=zlib.Z_HUFFMAN_ONLY)), ("rle", fq, dict(strategy=zlib.Z_RLE)),
             ("all_a", b"A" * 65280, {})]
    return [(name, text, member(text, **kw)) for name, text, kw in cases]


def periodic(period: int, nbytes: int = 20000) -> bytes:
    unit = bytes(np.random.default_rng(period).integers(65, 91, period, dtype=np.uint8))
    return (unit * (nbytes // period + 1))[:nbytes]


PERIODS = (1, 2, 3, 63, 64, 65, 257, 258, 259)


# ---- members assembled bit by bit ----------------------------------------------------------------------------------------

class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v: int, n: int):
        """n bits of v, least significant first (header fields, extra bits)."""
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, v: int, n: int):
        """A Huffman code of n bits, most significant first."""
        for k in range(n - 1, -1, -1):
            self.bits((v >> k) & 1, 1)

    def done(self) -> bytes:
        if self.n:
            self.bits(0, 8 - self.n)
        return bytes(self.out)


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class Fixed(BitWriter):
    """One final fixed-Huffman block."""

    def __init__(self):
        super().__init__()
        self.bits(1, 1)
        self.bits(1, 2)

    def sym(self, s: int):
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def lits(self, data: bytes):
        for b in data:
            self.sym(b)

    def dist_sym(self, d: int, extra: int = 0, nextra: int = 0):
        self.code(d, 5)
        self.bits(extra, nextra)

    def match(self, length: int, dist: int):
        ls = max(k for k in range(29) if LEN_BASE[k] <= length and (k == 28 or length != 258))
        self.sym(257 + ls)
        self.bits(length - LEN_BASE[ls], LEN_EXTRA[ls])
        ds = max(k for k in range(30) if DIST_BASE[k] <= dist)
        self.dist_sym(ds, dist - DIST_BASE[ds], DIST_EXTRA[ds])

    def end(self) -> bytes:
        self.sym(256)
        return self.done()


def hand_assembled():
    """[(name, text, member)]: fixed-Huffman members zlib cannot emit but must accept."""
    base = bytes(np.random.default_rng(9).integers(97, 123, 32768, dtype=np.uint8))
    out = []
    f = Fixed()
    f.lits(base)
    f.match(258, 32768)
    out.append(("len258_dist32768", base + base[:258], f.end()))
    f = Fixed()
    f.lits(b"x")
    f.match(3, 1)
    out.append(("len3_dist1", b"xxxx", f.end()))
    f = Fixed()
    f.lits(base)
    f.match(10, 16385 + 100)       # distance code 28
    f.match(10, 24577 + 5)         # distance code 29
    t = bytearray(base)
    for ln, d in ((10, 16485), (10, 24582)):
        for _ in range(ln):
            t.append(t[-d])
    out.append(("dist_codes_28_29", bytes(t), f.end()))
    res = []
    for name, text, payload in out:
        assert zlib.decompress(payload, -15) == text, name
        res.append((name, text, wrap(payload, zlib.crc32(text), len(text))))
    return res


# The code-length code of the hand-made dynamic headers: symbols 0..12 and 16, 17, 18 with four bits each (complete).
_CL_SYMS = list(range(13)) + [16, 17, 18]
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def dynamic_header(items, nlen: int, ndist: int, cl_lengths=None, cl_code=None) -> BitWriter:
    """A final dynamic block up to the end of its code lengths.  ``items``: code-length symbols, a length as an int
    (0..12 under the flat code), a repeat as (16 | 17 | 18, count).  ``cl_lengths``: {symbol: length} of another
    code-length code (then no items are written: the header is expected to fail before them).  ``cl_code``: a complete
    {symbol: length} code-length code, written and used for the items in place of the flat 4-bit one."""
    codes = None
    if cl_code is not None:
        assert cl_lengths is None and sum(1 << (7 - l) for l in cl_code.values()) == 128 and max(cl_code.values()) <= 7
        codes = _canonical([cl_code.get(s, 0) for s in range(19)])
    w = BitWriter()
    w.bits(1, 1)
    w.bits(2, 2)
    w.bits(nlen - 257, 5)
    w.bits(ndist - 1, 5)
    w.bits(19 - 4, 4)
    for s in _CL_ORDER:
        w.bits(cl_code.get(s, 0) if cl_code is not None else
               cl_lengths.get(s, 0) if cl_lengths is not None else (4 if s in _CL_SYMS else 0), 3)
    if cl_lengths is not None:
        return w
    for it in items:
        sym, rep = it if isinstance(it, tuple) else (it, None)
        if codes is None:
            w.code(_CL_SYMS.index(sym), 4)
        else:
            w.code(*codes[sym])
        if sym == 16:
            w.bits(rep - 3, 2)
        elif sym == 17:
            w.bits(rep - 3, 3)
        elif sym == 18:
            w.bits(rep - 11, 7)
    return w


def _lengths(nlen, ndist, lit, dist):
    """Items for explicit {symbol: length} maps, zeros in runs of symbol 18 / 17 where long enough."""
    full = [lit.get(s, 0) for s in range(nlen)] + [dist.get(s, 0) for s in range(ndist)]
    items, k = [], 0
    while k < len(full):
        run = 1
        while k + run < len(full) and full[k + run] == full[k] == 0 and run < 138:
            run += 1
        if full[k] == 0 and run >= 11:
            items.append((18, run))
        elif full[k] == 0 and run >= 3:
            items.append((17, run))
        else:
            items.append(full[k])
            run = 1
        k += run
    return items


def valid_dynamic():
    """[(name, text, member)]: hand-made dynamic blocks zlib accepts: a distance tree of one code, and of none."""
    out = []
    # literals 'a' (1 bit), 'b' (2), end (3), length symbol 257 (3); one distance code of length 1 (distance 1)
    w = dynamic_header(_lengths(258, 1, {97: 1, 98: 2, 256: 3, 257: 3}, {0: 1}), 258, 1)
    w.code(0b0, 1)      # a
    w.code(0b10, 2)     # b
    w.code(0b111, 3)    # length 3
    w.code(0, 1)        # distance 1
    w.code(0b110, 3)    # end
    out.append(("one_distance_code", b"abbbb", w.done()))
    w = dynamic_header(_lengths(257, 1, {97: 1, 256: 1}, {}), 257, 1)
    w.code(0, 1)
    w.code(0, 1)
    w.code(1, 1)
    out.append(("no_distance_code", b"aa", w.done()))
    res = []
    for name, text, payload in out:
        assert zlib.decompress(payload, -15) == text, name
        res.append((name, text, wrap(payload, zlib.crc32(text), len(text))))
    return res


# A complete code-length code on all 19 symbols with codes of 2 to 7 bits: the lengths 1..6 take 5 bits, 7..13 take 6,
# 14 and 15 take 7.
DEEP_CL_CODE = {0: 2, 18: 2, 17: 3, 16: 4, **{s: 5 for s in range(1, 7)}, **{s: 6 for s in range(7, 14)}, 14: 7, 15: 7}


class Dynamic:
    """One final dynamic block under the codes ``lit`` and ``dist`` ({symbol: length}), its header written with
    ``cl_code``; ``items``: the header's code-length items when they are not to be ``_lengths``'s."""

    def __init__(self, lit, dist, nlen=None, ndist=None, items=None, cl_code=DEEP_CL_CODE):
        nlen = max(257, max(lit) + 1) if nlen is None else nlen
        ndist = max(1, max(dist, default=0) + 1) if ndist is None else ndist
        items = _lengths(nlen, ndist, lit, dist) if items is None else items
        self.w = dynamic_header(items, nlen, ndist, cl_code=cl_code)
        self.lit = _canonical([lit.get(s, 0) for s in range(nlen)])
        self.dist = _canonical([dist.get(s, 0) for s in range(ndist)])
        self.text = bytearray()

    def lits(self, data: bytes):
        for b in data:
            self.w.code(*self.lit[b])
        self.text += data

    def match(self, length: int, dist: int, len_sym=None):
        """``len_sym``: the length symbol to use (258 has two: 285, and 284 with all five extra bits set)."""
        ls = len_sym - 257 if len_sym is not None else \
            max(k for k in range(29) if LEN_BASE[k] <= length and (k == 28 or length != 258))
        assert 0 <= length - LEN_BASE[ls] < max(1, 1 << LEN_EXTRA[ls])
        self.w.code(*self.lit[257 + ls])
        self.w.bits(length - LEN_BASE[ls], LEN_EXTRA[ls])
        ds = max(k for k in range(30) if DIST_BASE[k] <= dist)
        self.w.code(*self.dist[ds])
        self.w.bits(dist - DIST_BASE[ds], DIST_EXTRA[ds])
        for _ in range(length):
            self.text.append(self.text[-dist])
        return self.lit[257 + ls][1], self.dist[ds][1]

    def end(self):
        self.w.code(*self.lit[256])
        return bytes(self.text), self.w.done()


def deep_dynamic():
    """[(name, text, payload)]: hand-made dynamic blocks at the decoder's limits, which zlib accepts."""
    out = []
    # literal/length and distance codes of 1 .. 11, 13, 13, 14, 14 and four times 15 bits, the long ones in use
    lit = {**{97 + k: 1 + k for k in range(11)}, 108: 13, 109: 13, 256: 14, 284: 14, 285: 15, 257: 15, 110: 15, 111: 15}
    dist = {**{k: 1 + k for k in range(11)}, 11: 13, 12: 13, 13: 14, 14: 14, 26: 15, 27: 15, 28: 15, 29: 15}
    for with_284 in (False, True):
        d = Dynamic(lit, dist)
        d.lits(bytes(np.random.default_rng(41).choice(np.arange(97, 105, dtype=np.uint8), 32768,
                                                      p=[.5, .25, .125, .0625, .03125, .015625, .0078125, .0078125])))
        d.lits(bytes([108, 110, 109, 111]))                                  # 13, 15, 13 and 15 bits
        bits = [d.match(258, 32768), d.match(3, 49 + 15), d.match(3, 97 + 31), d.match(3, 16385 + 8191),
                d.match(258, 24577), d.match(3, 8193), d.match(3, 12289 + 4095)]
        assert {b[0] for b in bits} == {15} and {b[1] for b in bits} == {13, 14, 15}
        if with_284:
            assert d.match(258, 32768, len_sym=284) == (14, 15)             # 258 = 227 + 31
        out.append(("codes_of_13_14_15_bits" + ("_and_258_by_284" if with_284 else ""),) + d.end())
    # the repeat codes at their largest counts: 18 for 138 zeros, 16 for 6 more of the last length, 17 for 10 zeros, and
    # a 16 that runs from the last two literal/length lengths into the first five distance lengths
    items = [(18, 138), 3, (16, 6), (17, 10), (18, 101), 4, 5, (16, 6), 1, 2, 4, 5]
    lit = {**{s: 3 for s in range(138, 145)}, 256: 4, 257: 5, 258: 5}
    dist = {**{s: 5 for s in range(5)}, 5: 1, 6: 2, 7: 4, 8: 5}
    d = Dynamic(lit, dist, nlen=259, ndist=9, items=items)
    d.lits(bytes(range(138, 145)) * 3)
    for k, (n, far) in enumerate([(3, 1), (4, 2), (3, 3), (4, 4), (3, 5), (4, 7), (3, 9), (4, 13), (3, 17), (4, 21)]):
        d.match(n, far)
        d.lits(bytes([138 + k % 7]))
    out.append(("repeats_at_their_largest",) + d.end())
    # zlib decides what is a member: an entry it refuses is left out (258 by symbol 284 is the one in question)
    good = []
    for name, text, payload in out:
        try:
            if zlib.decompress(payload, -15) == text:
                good.append((name, text, payload))
                continue
        except zlib.error:
            pass
        assert name.endswith("_and_258_by_284"), name
    return good


def deep_codes():
    """[(name, text, member)] for the inflate at the code-length limits and the window's edge: the texts of
    tests/deflate_cases.py made for them, as members of this project's own encoder (both members of each) and of zlib at
    levels 1, 6 and 9, and the blocks of ``deep_dynamic``.  zlib inflates every one to its text before it is used."""
    from genefuserust_amd import deflate
    from tests import deflate_cases as dc
    out = []
    for name in ("window_edge", "deep_literals", "deep_distances", "deep_code_lengths", "every_symbol"):
        text = dc.texts()[name]
        for k in (0, 1):
            out.append(("%s_%d_own" % (name, k), text[k * dc.TEXT:(k + 1) * dc.TEXT],
                        deflate.deflate_member_host(text[k * dc.TEXT:(k + 1) * dc.TEXT])))
        out += [("%s_zlib_%d" % (name, level), text[:dc.TEXT], member(text[:dc.TEXT], level)) for level in (1, 6, 9)]
    out += [(name, text, wrap(payload, zlib.crc32(text), len(text))) for name, text, payload in deep_dynamic()]
    for name, text, m in out:
        assert zlib.decompress(m[18:-8], -15) == text and zlib.decompress(m, 31) == text, name
    return out


def parts(m: bytes):
    """(payload, crc, isize) of a member made by ``wrap`` without extra subfields."""
    crc, isize = struct.unpack("<II", m[-8:])
    return m[18:-8], crc, isize


def malformed():
    """[(name, member, status)]: every way of §1 in which a member can be wrong, each made from a valid member or
    header.  The members keep well-formed BGZF framing, so that they walk like any other."""
    fq = fastq_text(3000, seed=3)
    out = []

    def edit(name, status, m, payload=None, crc=None, isize=None):
        p, c, n = parts(m)
        out.append((name, wrap(p if payload is None else payload, c if crc is None else crc, n if isize is None else isize),
                    status))

    def flip(p, i, mask_clear, value):
        b = bytearray(p)
        b[i] = (b[i] & ~mask_clear & 255) | value
        return bytes(b)

    one, stored, dyn = member(b"G"), member(fq, level=0), member(fq, level=6)
    assert block_kinds(parts(one)[0])[0] == 1 and block_kinds(parts(stored)[0])[0] == 0 and block_kinds(parts(dyn)[0])[0] == 2
    edit("btype_3", BAD_BTYPE, one, flip(parts(one)[0], 0, 0x06, 0x06))
    edit("stored_nlen", STORED_LEN, stored, flip(parts(stored)[0], 3, 0x01, ~parts(stored)[0][3] & 1))
    edit("hlit_287", BAD_COUNTS, dyn, flip(parts(dyn)[0], 0, 0xf8, 30 << 3))
    edit("hdist_31", BAD_COUNTS, dyn, flip(parts(dyn)[0], 1, 0x1f, 30))
    edit("hdist_32", BAD_COUNTS, dyn, flip(parts(dyn)[0], 1, 0x1f, 31))

    def header(name, status, w, isize=4):
        out.append((name, wrap(w.done() + b"\0" * 8, 0, isize), status))
    header("code_length_code_oversubscribed", OVERSUBSCRIBED, dynamic_header([], 257, 1, {0: 1, 1: 1, 2: 1}))
    header("code_length_code_incomplete", INCOMPLETE, dynamic_header([], 257, 1, {0: 2, 1: 2}))
    header("literal_code_oversubscribed", OVERSUBSCRIBED,
           dynamic_header(_lengths(257, 1, {97: 1, 98: 1, 256: 1}, {0: 1}), 257, 1))
    header("literal_code_incomplete", INCOMPLETE, dynamic_header(_lengths(257, 1, {97: 2, 256: 2}, {0: 1}), 257, 1))
    header("literal_code_of_one_code", INCOMPLETE, dynamic_header(_lengths(257, 1, {256: 1}, {0: 1}), 257, 1), isize=0)
    header("distance_code_oversubscribed", OVERSUBSCRIBED,
           dynamic_header(_lengths(257, 3, {97: 1, 256: 1}, {0: 1, 1: 1, 2: 1}), 257, 3))
    header("distance_code_incomplete", INCOMPLETE, dynamic_header(_lengths(257, 2, {97: 1, 256: 1}, {0: 2, 1: 2}), 257, 2))
    header("repeat_16_first", REPEAT_FIRST, dynamic_header([(16, 3)], 257, 1))
    header("lengths_overrun", LENGTHS_OVERRUN, dynamic_header([1, (18, 138), (18, 138)], 257, 1))
    header("lengths_overrun_by_16", LENGTHS_OVERRUN, dynamic_header([1, (18, 138), (18, 116), 1, (16, 6)], 257, 1))
    header("no_end_code", NO_END_CODE, dynamic_header(_lengths(257, 1, {97: 1, 98: 1}, {0: 1}), 257, 1))
    # a distance code of one code: the other bit is no code
    w = dynamic_header(_lengths(258, 1, {97: 1, 98: 2, 256: 3, 257: 3}, {0: 1}), 258, 1)
    w.code(0b0, 1)
    w.code(0b111, 3)
    w.code(1, 1)
    header("bit_outside_the_one_distance_code", BAD_CODE, w)
    # a match with no distance code at all
    w = dynamic_header(_lengths(258, 1, {97: 1, 256: 2, 257: 2}, {}), 258, 1)
    w.code(0b0, 1)
    w.code(0b11, 2)
    header("match_without_distance_codes", BAD_CODE, w)

    def fixed(name, status, build, isize):
        f = Fixed()
        build(f)
        out.append((name, wrap(f.end(), 0, isize), status))
    fixed("litlen_286", BAD_LITLEN, lambda f: (f.lits(b"ab"), f.sym(286), f.dist_sym(0)), 8)
    fixed("litlen_287", BAD_LITLEN, lambda f: (f.lits(b"ab"), f.sym(287), f.dist_sym(0)), 8)
    fixed("dist_30", BAD_DIST_SYM, lambda f: (f.lits(b"ab"), f.sym(257), f.dist_sym(30)), 8)
    fixed("dist_31", BAD_DIST_SYM, lambda f: (f.lits(b"ab"), f.sym(257), f.dist_sym(31)), 8)
    fixed("distance_past_the_start", DIST_TOO_FAR, lambda f: (f.lits(b"a"), f.match(3, 2)), 4)
    fixed("distance_at_the_very_start", DIST_TOO_FAR, lambda f: f.match(3, 1), 3)
    edit("isize_one_less_literal", OUTPUT_OVERRUN, member(fq, strategy=zlib.Z_HUFFMAN_ONLY), isize=len(fq) - 1)
    edit("isize_one_less_match", OUTPUT_OVERRUN, member(b"A" * 3000), isize=2999)
    edit("stored_isize_one_less", OUTPUT_OVERRUN, stored, isize=len(fq) - 1)
    edit("isize_one_more", OUTPUT_SHORT, dyn, isize=len(fq) + 1)
    edit("isize_zero", OUTPUT_OVERRUN, dyn, isize=0)
    p = parts(dyn)[0]
    edit("payload_cut_in_half", INPUT_EXHAUSTED, dyn, p[:len(p) // 2])
    edit("payload_cut_in_the_header", INPUT_EXHAUSTED, dyn, p[:5])
    edit("payload_empty", INPUT_EXHAUSTED, dyn, b"")
    edit("stored_payload_cut", INPUT_EXHAUSTED, stored, parts(stored)[0][:100])
    edit("crc_flipped", CRC, dyn, crc=parts(dyn)[1] ^ 1)
    edit("crc_of_other_text", CRC, member(b"A" * 3000), crc=zlib.crc32(b"B" * 3000))
    edit("payload_with_a_byte_behind", TRAILING, dyn, p + b"\0")
    return out


# ---- what a dynamic block is made of ------------------------------------------------------------------------------------

def _canonical(lengths):
    """{symbol: (code, length)} of the canonical code of ``lengths`` (RFC 1951, 3.2.2)."""
    code, out = 0, {}
    for n in range(1, 16):
        for s, l in enumerate(lengths):
            if l == n:
                out[s] = (code, n)
                code += 1
        code <<= 1
    return out


def _decode_table(lengths):
    """For every 15 bits of the stream, first bit least significant: symbol << 4 | code length (0: no code)."""
    table = np.zeros(1 << 15, dtype=np.int32)
    for s, (code, n) in _canonical(lengths).items():
        rev = int(format(code, "0%db" % n)[::-1], 2)
        table[rev::1 << n] = (s << 4) | n
    return table.tolist()


def tokens_of(payload: bytes):
    """A raw DEFLATE payload of one final dynamic block, taken apart: (literal/length code lengths [HLIT], distance code
    lengths [HDIST], code-length code lengths [19], tokens), a token a byte value or (length, distance).  Independent of
    the decoder under test; ``replay`` turns the tokens back into text."""
    bits = np.unpackbits(np.frombuffer(payload + b"\0" * 4, dtype=np.uint8), bitorder="little").astype(np.int32)
    peek = np.zeros(len(bits), dtype=np.int32)
    for k in range(15):
        peek[:len(bits) - k] |= bits[k:] << k
    peek = peek.tolist()
    assert peek[0] & 7 == 0b101, "one final dynamic block"
    hlit, hdist, hclen = 257 + (peek[3] & 31), 1 + (peek[8] & 31), 4 + (peek[13] & 15)
    pos, cl = 17, [0] * 19
    for k in range(hclen):
        cl[_CL_ORDER[k]] = peek[pos] & 7
        pos += 3
    table, lengths = _decode_table(cl), []
    while len(lengths) < hlit + hdist:
        e = table[peek[pos] & 0x7fff]
        assert e & 15, "bits that are no code of the code-length code"
        pos += e & 15
        s = e >> 4
        if s < 16:
            lengths.append(s)
        else:
            nbits, base = {16: (2, 3), 17: (3, 3), 18: (7, 11)}[s]
            lengths += [lengths[-1] if s == 16 else 0] * (base + (peek[pos] & ((1 << nbits) - 1)))
            pos += nbits
    assert len(lengths) == hlit + hdist
    lit, dist = lengths[:hlit], lengths[hlit:]
    lit_table, dist_table, tokens = _decode_table(lit), _decode_table(dist), []
    while True:
        e = lit_table[peek[pos] & 0x7fff]
        assert e & 15, "bits that are no literal/length code"
        pos += e & 15
        s = e >> 4
        if s < 256:
            tokens.append(s)
            continue
        if s == 256:
            break
        n = LEN_EXTRA[s - 257]
        length = LEN_BASE[s - 257] + (peek[pos] & ((1 << n) - 1))
        pos += n
        e = dist_table[peek[pos] & 0x7fff]
        assert e & 15, "bits that are no distance code"
        pos += e & 15
        n = DIST_EXTRA[e >> 4]
        tokens.append((length, DIST_BASE[e >> 4] + (peek[pos] & ((1 << n) - 1))))
        pos += n
    assert (pos + 7) // 8 == len(payload), "the block ends in the payload's last byte"
    return lit, dist, cl, tokens


def replay(tokens) -> bytes:
    out = bytearray()
    for t in tokens:
        if isinstance(t, tuple):
            assert 1 <= t[1] <= len(out)
            for _ in range(t[0]):
                out.append(out[-t[1]])
        else:
            out.append(t)
    return bytes(out)


def token_symbols(tokens):
    """(literal/length counts [286] with the end-of-block symbol, distance counts [30]) of a block's tokens."""
    lit, dist = [0] * 286, [0] * 30
    lit[256] = 1
    for t in tokens:
        if isinstance(t, tuple):
            lit[257 + (28 if t[0] == 258 else max(k for k in range(28) if LEN_BASE[k] <= t[0]))] += 1
            dist[max(k for k in range(30) if DIST_BASE[k] <= t[1])] += 1
        else:
            lit[t] += 1
    return lit, dist


# ---- the walk ---------------------------------------------------------------------------------------------------------------

def walk_model(comp: bytes, file_offset: int = 0, text_budget: int = 1 << 62, max_members: int = 1 << 30):
    """gf_if_walk_blocks in Python: (rows [[payload offset, payload length, text offset, text length, CRC-32, offset in
    the file]], compressed bytes of the whole members, their text bytes, why it stopped, the offset in ``comp`` where it
    stopped)."""
    rows, off, text = [], 0, 0
    n = len(comp)
    while True:
        if off == n:
            return rows, off, text, WALK_END, off
        head = comp[off:off + 4]
        if head != b"\x1f\x8b\x08\x04"[:len(head)]:
            return rows, off, text, WALK_NOT_BGZF, off
        if n - off < 12:
            return rows, off, text, WALK_INSIDE, off
        xlen, = struct.unpack_from("<H", comp, off + 10)
        if n - off < 12 + xlen:
            return rows, off, text, WALK_INSIDE, off
        p, end, bsize = off + 12, off + 12 + xlen, None
        while p + 4 <= end:
            slen, = struct.unpack_from("<H", comp, p + 2)
            if comp[p:p + 2] == b"BC" and slen == 2 and p + 6 <= end:
                bsize = struct.unpack_from("<H", comp, p + 4)[0] + 1
                break
            p += 4 + slen
        if bsize is None or bsize < 12 + xlen + 8:
            return rows, off, text, WALK_NOT_BGZF, off
        if n - off < bsize:
            return rows, off, text, WALK_INSIDE, off
        crc, isize = struct.unpack_from("<II", comp, off + bsize - 8)
        if isize > MAX_TEXT:
            return rows, off, text, WALK_NOT_BGZF, off
        if text + isize > text_budget:
            return rows, off, text, WALK_BUDGET, off
        if len(rows) >= max_members:
            return rows, off, text, WALK_CAPACITY, off
        rows.append([off + 12 + xlen, bsize - xlen - 20, text, isize, crc, file_offset + off])
        off += bsize
        text += isize


def table_of(members, text_gap: int = 0, comp_gap: int = 0, text_base: int = 0):
    """(compressed buffer, int64 table, output bytes needed) for members laid out back to back with ``comp_gap`` bytes
    between them in the compressed buffer and ``text_gap`` between their texts — odd gaps put them at odd offsets."""
    comp, rows, t = bytearray(), [], text_base
    for m in members:
        comp += b"\xEE" * comp_gap
        walked, _, _, why, _ = walk_model(bytes(m))
        assert why == WALK_END and len(walked) == 1
        r = walked[0]
        rows.append([r[0] + len(comp), r[1], t, r[3], r[4], len(comp)])
        comp += m
        t += r[3] + text_gap
    return bytes(comp), np.asarray(rows, dtype=np.int64).reshape(-1, ROW), t
