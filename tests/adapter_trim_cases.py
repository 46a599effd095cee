"""The reads that the adapter trimming's tests share (tests/test_adapter_trim_core.py on the host,
tests/test_adapter_trim_gpu.py on the device): pairs and single-end reads at every edge of the predicate of
include/gf_adapter_trim.h, and random ones.  Built once per settings and left unchanged; the model's answers are
computed once per settings too (``modelled``)."""
import functools
from typing import List, Optional, Tuple

import numpy as np

from tests.adapter_trim_model import TRUSEQ_R1, TRUSEQ_R2, Settings, decide

LENGTHS = [0, 1, 29, 30, 31, 32, 33, 63, 64, 65, 127, 128, 129, 150, 151, 255, 256, 257, 512, 513, 4100]
Pair = Tuple[bytes, bytes]

# the settings the kernel is held to the model on
SETTINGS = {
    "defaults": Settings(),
    "illumina": Settings(adapter_r1=TRUSEQ_R1, adapter_r2=TRUSEQ_R2),
    "sequence only": Settings(overlap=0, adapter_r1=TRUSEQ_R1, adapter_r2=TRUSEQ_R2[:12]),
    "percent 10": Settings(diff_percent=10, adapter_r1=TRUSEQ_R1),
    "percent bites": Settings(max_diff=10, adapter_r2=TRUSEQ_R2),
    "smallest": Settings(min_overlap=8, max_diff=0, diff_percent=0, min_adapter=4, adapter_r1=b"ACGT",
                         adapter_r2=b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT" + b"ACGTTGCA" * 3 + b"ACGTACG"),
}
assert len(SETTINGS["smallest"].adapter_r2) == 64


def rc(x: bytes) -> bytes:
    return x.translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]


def bases_of(rng, n: int) -> bytes:
    return rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tobytes()


def quals_of(b: bytes) -> bytes:
    """Qualities that differ from position to position, so that a prefix is recognised as one."""
    return bytes(33 + (7 * i + len(b)) % 41 for i in range(len(b)))


def other_base(c: int) -> int:
    return b"CGTA"[b"ACGT".index(bytes([c]).upper())]


def with_diffs(x: bytes, where) -> bytes:
    out = bytearray(x)
    for i in where:
        out[i] = other_base(out[i])
    return bytes(out)


def read_through(rng, insert: bytes, L1: int, L2: int, s: Settings, a1: Optional[bytes] = None,
                 a2: Optional[bytes] = None) -> Pair:
    """The mates of a fragment: the insert, then each mate's adapter (the settings', or TruSeq), then random bases."""
    a1 = (s.adapter_r1 or TRUSEQ_R1) if a1 is None else a1
    a2 = (s.adapter_r2 or TRUSEQ_R2) if a2 is None else a2
    return (insert + a1 + bases_of(rng, L1))[:L1], (rc(insert) + a2 + bases_of(rng, L2))[:L2]


def spread(rng, lo: int, hi: int, k: int) -> List[int]:
    """k distinct positions of [lo, hi)."""
    return sorted(int(x) for x in rng.choice(np.arange(lo, hi), k, replace=False))


def tandem_pair(rng, s: Settings) -> Pair:
    """An insert of 98 bases that repeats with period 7, read through by mates of 120 bases."""
    unit = b"ACGGTCA"
    return read_through(rng, unit * 14, 120, 120, s)


def edge_pairs(s: Settings, seed: int = 1) -> List[Pair]:
    rng = np.random.default_rng(seed)
    mo, out = s.min_overlap, []
    L = 150
    # inserts around min_overlap, around the read length, and at the last candidate and one above
    for I in (mo - 1, mo, mo + 1, L - 1, L, L + 1, 2 * L - mo, 2 * L - mo + 1, 166, 100):
        out.append(read_through(rng, bases_of(rng, I), L, L, s))
    # planted differences: none, max_diff, one more; inside the overlap of an insert of 100 and of exactly min_overlap
    for I in (100, mo, 40):
        for k in sorted({0, 1, 3, 4, s.max_diff, s.max_diff + 1, 6, 7, 10, 11} - {k for k in range(12) if k > I}):
            a, b = read_through(rng, bases_of(rng, I), L, L, s)
            out.append((with_diffs(a, spread(rng, 0, I, k)), b))
            out.append((a, with_diffs(b, spread(rng, 0, I, k))))
    # N and lower case inside the overlap
    for I in (100, 166):
        a, b = read_through(rng, bases_of(rng, I), L, L, s)
        ov0 = max(0, I - L)
        out.append((a[:ov0 + 5] + a[ov0 + 5:ov0 + 30].lower() + a[ov0 + 30:], b.lower()))
        for k in (1, s.max_diff, s.max_diff + 1):
            n_at = spread(rng, ov0, min(I, L), k)
            out.append((bytes(ord("N") if i in n_at else c for i, c in enumerate(a)), b))
            out.append((a, bytes(ord("n") if I - 1 - i in n_at else c for i, c in enumerate(b))))
    # mates of different lengths
    for L1, L2, I in ((150, 100, 80), (100, 150, 120), (150, 40, 60), (33, 150, 100), (150, 31, 150), (64, 65, 64),
                      (512, 30, 300), (30, 512, 29)):
        out.append(read_through(rng, bases_of(rng, I), L1, L2, s))
    out.append(tandem_pair(rng, s))
    # every length: a read-through pair, a pair that overlaps end to end, and a pair of unrelated reads
    for n in LENGTHS:
        out.append(read_through(rng, bases_of(rng, max(n * 2 // 3, 1)), n, n, s))
        whole = bases_of(rng, n)
        out.append((whole, rc(whole)))
        out.append((bases_of(rng, n), bases_of(rng, min(n, 150))))
    out.append((bases_of(rng, 150), b""))
    out.append((b"", bases_of(rng, 150)))
    out.append((bases_of(rng, 513), bases_of(rng, 100)))
    # no I*: the adapter of each mate, and all A
    for n in (60, 150):
        out.append((b"A" * n, b"A" * n))
        out.append((b"A" * n, b"T" * n))
        a, _ = read_through(rng, bases_of(rng, n - 20), n, n, s)
        _, b = read_through(rng, bases_of(rng, n - 25), n, n, s)
        out.append((a, b))
    return out + [(a, b) for a in adapter_reads(s, 0, seed + 1)[::7] for b in adapter_reads(s, 1, seed + 2)[::11]][:40]


def adapter_reads(s: Settings, side: int = 0, seed: int = 3) -> List[bytes]:
    """Single reads around the sequence step: the adapter of ``side`` starting at every p from L - nA - 3 to
    L - min_adapter + 1 with no, floor(n / 10) and floor(n / 10) + 1 differences; p = 0; every length; all A."""
    rng = np.random.default_rng(seed)
    adapter = (s.adapter_r1, s.adapter_r2)[side] or (TRUSEQ_R1, TRUSEQ_R2)[side]
    nA, out = len(adapter), []
    for L in (100, 150):
        for p in range(max(L - nA - 3, 0), L - s.min_adapter + 2):
            n = min(nA, L - p)
            for k in sorted({0, n // 10, n // 10 + 1}):
                body = bytearray((bases_of(rng, p) + adapter + bases_of(rng, L))[:L])
                for j in spread(rng, 0, n, min(k, n)):
                    body[p + j] = other_base(body[p + j])
                out.append(bytes(body))
        hit = (bases_of(rng, L - 40) + adapter + bases_of(rng, L))[:L]
        out.append(hit.lower())
        out.append(hit[:L - 38] + b"N" + hit[L - 37:])
        out.append(hit[:L - 38] + b"NNNNN" + hit[L - 33:])
    for L in LENGTHS:
        out.append((adapter + bases_of(rng, L))[:L])                         # p = 0: an adapter dimer
        out.append((bases_of(rng, L // 2) + adapter + bases_of(rng, L))[:L])
        out.append(bases_of(rng, L))
        out.append(b"A" * L)
    return out


def random_pairs(n: int, seed: int, s: Settings = Settings(), longest: int = 150) -> List[Pair]:
    """Fragments of 20 to 2.2 read lengths read by mates of differing lengths, one base in 50 flipped."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        L1, L2 = (int(x) for x in rng.integers(longest // 3, longest + 1, 2))
        a, b = read_through(rng, bases_of(rng, int(rng.integers(20, longest * 22 // 10))), L1, L2, s)
        flip = lambda x: with_diffs(x, np.nonzero(rng.random(len(x)) < 0.02)[0])   # noqa: E731
        out.append((flip(a), flip(b)))
    return out


@functools.lru_cache(maxsize=None)
def pair_cases(name: str) -> Tuple[Pair, ...]:
    return tuple(edge_pairs(SETTINGS[name]) + random_pairs(90, 17, SETTINGS[name], 90))


@functools.lru_cache(maxsize=None)
def single_cases(name: str) -> Tuple[bytes, ...]:
    return tuple(adapter_reads(SETTINGS[name]))


@functools.lru_cache(maxsize=None)
def modelled(name: str, single: bool = False):
    """The model's verdicts of ``pair_cases(name)`` (or of ``single_cases(name)``), computed once."""
    s = SETTINGS[name]
    if single:
        return tuple(tuple(decide(a, None, s)) for a in single_cases(name))
    return tuple(tuple(decide(a, b, s)) for a, b in pair_cases(name))
