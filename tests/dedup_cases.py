"""The records libgfdedup.so is held to, shared by the host and the device tests: a read of every length at which the
walk of a record changes (a word, a piece, a round, GF_MAX_READ_LEN and past it), near-duplicates that must get other
keys, and batches with a known share of repeats."""
import functools

import numpy as np

LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 150, 255, 256, 257, 4096, 5000]
JUNK = [0, 0xFF, ord("G"), ord("a"), 0x20]   # (0x20: the bit that fold drops)
ALPHABET = np.frombuffer(b"ACGTACGTACGTacgtN", dtype=np.uint8)


def random_read(rng, n: int) -> bytes:
    return rng.choice(ALPHABET, n).tobytes()


@functools.lru_cache(maxsize=None)
def edge_reads():
    """Two reads of every length of ``LENGTHS`` (one of length 0 would do; two keep the pairing simple)."""
    rng = np.random.default_rng(11)
    return tuple(random_read(rng, n) for n in LENGTHS for _ in range(2))


def swap_case(b: bytes) -> bytes:
    return bytes(c ^ 0x20 if chr(c).isalpha() else c for c in b)


@functools.lru_cache(maxsize=None)
def near_duplicates():
    """(record, other record, whether the keys must be equal): a trailing NUL byte, one base anywhere, the case."""
    out = []
    for b in edge_reads()[::2]:
        out.append((b, b + b"\0", False))
        out.append((b, swap_case(b), True))
        for at in sorted({0, len(b) // 2, len(b) - 1} if b else ()):
            other = bytearray(b)
            other[at] = ord("T") if other[at] & 0xDF != ord("T") else ord("A")
            out.append((b, bytes(other), False))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def mixed_reads():
    """Reads of up to 600 bases for the batches: the edge lengths below that, and short random ones; a quarter of
    them repeats of an earlier one, some in the other case."""
    rng = np.random.default_rng(12)
    reads = [r for r in edge_reads() if len(r) <= 600] + [random_read(rng, int(n)) for n in rng.integers(0, 200, 80)]
    out = []
    for k, r in enumerate(reads):
        out.append(r)
        if k % 4 == 1:
            out.append(reads[int(rng.integers(0, k))])
        if k % 8 == 3:
            out.append(swap_case(reads[int(rng.integers(0, k))]))
    return tuple(out)


def batch_reads(n: int, salt: int = 0):
    """``n`` reads of ``mixed_reads``, walked with a stride so that repeats land at every distance."""
    cases = mixed_reads()
    return [cases[(7 * (n + salt) + 3 * k) % len(cases)] for k in range(n)]


def batch_pairs(n: int, salt: int = 0):
    """``n`` pairs: the mates drawn independently, so that pairs repeat only when both do; every eighth pair has an
    empty R2, every sixteenth an empty R1, and pair 5 (when there is one) is empty on both sides."""
    left, right = batch_reads(n, salt), batch_reads(n, salt + 5)[::-1]
    pairs = []
    for k, (a, b) in enumerate(zip(left, right)):
        if k % 4 == 2 and k >= 2:
            a, b = pairs[k - 2 if k % 8 == 2 else k // 2]   # a repeat: adjacent-but-one, or far back
        if k % 8 == 7:
            b = b""
        if k % 16 == 9:
            a = b""
        if k == 5:
            a = b = b""
        pairs.append((a, b))
    return pairs
