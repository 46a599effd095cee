"""The pairs that the overlap correction's tests share (tests/test_overlap_correct_core.py on the host,
tests/test_overlap_correct_gpu.py on the device): pairs at every edge of the predicate of
include/gf_overlap_correct.h, and random ones.  Built once per settings and left unchanged; the model's answers are
computed once per settings too (``modelled``).  A case is (a, qa, b, qb)."""
import functools
from typing import List, Tuple

import numpy as np

from tests.adapter_trim_cases import LENGTHS, bases_of, other_base, random_pairs, rc, read_through, spread, tandem_pair
from tests.adapter_trim_model import Settings as TrimSettings
from tests.overlap_correct_model import Corrected, Settings, correct_pair

Case = Tuple[bytes, bytes, bytes, bytes]

# the settings the kernel is held to the model on
SETTINGS = {
    "defaults": Settings(),
    "phred 20 10": Settings(good_phred=20, bad_phred=10),
    "smallest overlap": Settings(min_overlap=8, max_diff=2, diff_percent=25, good_phred=35, bad_phred=2),
    "wide": Settings(max_diff=10, diff_percent=100, good_phred=1, bad_phred=0),
}
TRIM = TrimSettings()   # (read_through takes the adapters from it: TruSeq)


def good_q(s: Settings) -> int:
    """A quality byte well above ``good_phred``."""
    return 33 + min(s.good_phred + 5, 93)


def bad_q(s: Settings) -> int:
    """A quality byte at or below ``bad_phred``."""
    return 33 + max(s.bad_phred - 3, 0)


class Pair:
    """A read-through pair of the insert length I with good qualities everywhere, and miscalls planted into it."""

    def __init__(self, rng, s: Settings, I: int, L1: int = 150, L2: int = 150, pair=None):
        a, b = read_through(rng, bases_of(rng, I), L1, L2, TRIM) if pair is None else pair
        self.I, self.s = I, s
        self.a, self.b = bytearray(a), bytearray(b)
        self.qa, self.qb = bytearray([good_q(s)] * len(a)), bytearray([good_q(s)] * len(b))
        self.lo, self.hi = max(0, I - len(b)), min(I, len(a))

    def miscall(self, i: int, side: int, q_low=None, q_high=None, base=None) -> "Pair":
        """A difference at a's position i: the base of ``side`` (0: a[i], 1: b[I - 1 - i]) is flipped (or becomes
        ``base``) and gets the quality ``q_low``; the base it faces gets ``q_high``."""
        j = self.I - 1 - i
        assert self.lo <= i < self.hi and 0 <= j < len(self.b)
        x, q, k = ((self.a, self.qa, i), (self.b, self.qb, j))[side]
        y, p, m = ((self.b, self.qb, j), (self.a, self.qa, i))[side]
        x[k] = other_base(x[k]) if base is None else base
        q[k] = bad_q(self.s) if q_low is None else q_low
        p[m] = good_q(self.s) if q_high is None else q_high
        return self

    def case(self) -> Case:
        return bytes(self.a), bytes(self.qa), bytes(self.b), bytes(self.qb)


def edge_cases(s: Settings, seed: int = 5) -> List[Case]:
    rng = np.random.default_rng(seed)
    good, bad = 33 + s.good_phred, 33 + s.bad_phred
    out = []
    # the thresholds: the source exactly good_phred and one below, the corrected base exactly bad_phred and one above
    for side in (0, 1):
        for q_high in (good, good - 1):
            for q_low in (bad, bad + 1):
                out.append(Pair(rng, s, 100).miscall(40, side, q_low, q_high).case())
    # both good, both bad: left standing
    out.append(Pair(rng, s, 100).miscall(41, 0, good_q(s), good_q(s)).case())
    out.append(Pair(rng, s, 100).miscall(41, 1, bad_q(s), bad_q(s)).case())
    # a quality byte below 33 is phred 0: as the corrected base's, and as the would-be source's
    for side in (0, 1):
        out.append(Pair(rng, s, 100).miscall(42, side, 10).case())
        out.append(Pair(rng, s, 100).miscall(42, side, 0, 32).case())
    # a low N against a good base is corrected; a good N is never a source
    for side in (0, 1):
        for n in (ord("N"), ord("n"), ord(".")):
            out.append(Pair(rng, s, 100).miscall(43, side, base=n).case())
        p = Pair(rng, s, 100).miscall(44, side, good_q(s), bad_q(s), base=ord("N"))   # (the N is good, its mate's base bad)
        out.append(p.case())
    # a lower-case source is written upper case; a lower-case miscall is a difference like any other
    for side in (0, 1):
        p = Pair(rng, s, 100)
        p.a, p.b = bytearray(bytes(p.a).lower()), bytearray(bytes(p.b).lower())
        out.append(p.miscall(45, side).case())
    # differences at lo, hi - 1 and around the word boundaries, with I* below and above the read length
    for I in (100, 166):
        for side in (0, 1):
            lo, hi = max(0, I - 150), min(I, 150)
            for i in sorted({lo, hi - 1, 31, 32, 63, 64, 95, 96} & set(range(lo, hi))):
                out.append(Pair(rng, s, I).miscall(i, side).case())
    # I* below, at and above the read length; mates of different lengths
    for L1, L2, I in ((150, 150, 149), (150, 150, 150), (150, 150, 151), (150, 100, 80), (100, 150, 120), (150, 40, 60),
                      (33, 150, 100), (150, 31, 150), (64, 65, 64), (512, 30, 300), (30, 512, 290), (129, 257, 200),
                      (257, 129, 300), (512, 512, 512), (512, 512, 700), (255, 256, 40)):
        p = Pair(rng, s, I, L1, L2)
        p.miscall(p.lo, 0).miscall(p.hi - 1, 1)
        if p.hi - p.lo > 4:
            p.miscall(p.lo + 2, 1)
        out.append(p.case())
    # d = max_diff: all corrected; one more: no I*, the pair is untouched
    for k in (s.max_diff, s.max_diff + 1):
        p = Pair(rng, s, 100)
        for n, i in enumerate(spread(rng, 0, 100, k)):
            p.miscall(i, n & 1)
        out.append(p.case())
    # the tandem-repeat pair: several accepted inserts, the correction is at the largest
    p = Pair(rng, s, 98, pair=tandem_pair(rng, TRIM))
    out.append(p.miscall(50, 0).miscall(60, 1).case())
    # both mates corrected in one pair, and a difference left standing beside them
    out.append(Pair(rng, s, 120).miscall(10, 0).miscall(70, 1).miscall(90, 0, good_q(s), good_q(s)).case())
    # nothing to do: no difference; no overlap; a mate of length 0; a mate too long; every length end to end
    out.append(Pair(rng, s, 100).case())
    for n in LENGTHS:
        whole = bases_of(rng, n)
        for a, b in ((whole, rc(whole)), (bases_of(rng, n), bases_of(rng, min(n, 150)))):
            out.append((a, bytes([bad_q(s)] * len(a)), b, bytes([good_q(s)] * len(b))))
    for a, b in ((bases_of(rng, 150), b""), (b"", bases_of(rng, 150)), (bases_of(rng, 513), bases_of(rng, 100))):
        out.append((a, bytes([good_q(s)] * len(a)), b, bytes([bad_q(s)] * len(b))))
    return out


def random_cases(n: int, s: Settings, seed: int = 23) -> List[Case]:
    """Random read-through pairs with one base in 50 flipped, under qualities drawn around the two thresholds."""
    rng = np.random.default_rng(seed)
    levels = np.array(sorted({20, 33, 33 + s.bad_phred, 34 + s.bad_phred, 32 + s.good_phred, 33 + s.good_phred,
                              bad_q(s), good_q(s)}), dtype=np.uint8)
    out = []
    for a, b in random_pairs(n, seed + 1, TRIM, 90):
        out.append((a, rng.choice(levels, len(a)).tobytes(), b, rng.choice(levels, len(b)).tobytes()))
    return out


@functools.lru_cache(maxsize=None)
def cases(name: str) -> Tuple[Case, ...]:
    return tuple(edge_cases(SETTINGS[name]) + random_cases(150, SETTINGS[name]))


@functools.lru_cache(maxsize=None)
def modelled(name: str) -> Tuple[Corrected, ...]:
    """The model's answers of ``cases(name)``, computed once."""
    return tuple(correct_pair(*c, SETTINGS[name]) for c in cases(name))
