"""The predicate of include/gf_adapter_trim.h as plain loops over bytes, written from the header's text: what the host
program (tests/test_adapter_trim_core.py) and the kernels (tests/test_adapter_trim_gpu.py) are held to.  No packing, no
search order: every candidate is tested, one base at a time."""
from typing import List, NamedTuple, Optional, Sequence, Tuple

UNTOUCHED, BY_OVERLAP, BY_SEQUENCE, OVERLAP_CLEAN = 0, 1, 2, 3
READ_MAX = 512
TRUSEQ_R1 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
TRUSEQ_R2 = b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"
TOTAL_KEYS = ("reads_seen", "adapter_reads_cut", "adapter_bases_cut", "adapter_cut_by_overlap",
              "adapter_cut_by_sequence", "adapter_overlapping_pairs")
PARTNER = {"A": "T", "T": "A", "C": "G", "G": "C"}


class Settings(NamedTuple):
    overlap: int = 1
    min_overlap: int = 30
    max_diff: int = 5
    diff_percent: int = 20
    min_adapter: int = 10
    adapter_r1: bytes = b""
    adapter_r2: bytes = b""


def complementary(x: int, y: int) -> bool:
    return PARTNER.get(chr(x).upper()) == chr(y).upper()


def overlap_diff(a: bytes, b: bytes, insert: int) -> Tuple[int, int]:
    """(ov(I), d(I))."""
    lo, hi = max(0, insert - len(b)), min(insert, len(a))
    return hi - lo, sum(1 for i in range(lo, hi) if not complementary(a[i], b[insert - 1 - i]))


def accepted_inserts(a: bytes, b: bytes, s: Settings) -> List[int]:
    """Every accepted I, ascending.  (``overlap_diff`` with the bases looked up once: a base of a as 0 .. 3 or -1, a
    base of b as the number of its partner or -2.)"""
    ca = ["ACGT".find(chr(x).upper()) for x in a]
    pb = [3 - "ACGT".find(chr(y).upper()) if chr(y).upper() in "ACGT" else -2 for y in b]
    out = []
    for insert in range(s.min_overlap, len(a) + len(b) - s.min_overlap + 1):
        lo, hi = max(0, insert - len(b)), min(insert, len(a))
        ov, d = hi - lo, 0
        for i in range(lo, hi):
            if ca[i] != pb[insert - 1 - i]:
                d += 1
        if ov >= s.min_overlap and d <= s.max_diff and 100 * d <= s.diff_percent * ov:
            out.append(insert)
    return out


def adapter_position(x: bytes, adapter: bytes, s: Settings) -> Optional[int]:
    """The smallest p at which the adapter lies in x, None without one."""
    if not adapter:
        return None
    for p in range(0, len(x) - s.min_adapter + 1):
        n = min(len(adapter), len(x) - p)
        d = sum(1 for j in range(n) if chr(x[p + j]).upper() not in "ACGT" or chr(x[p + j]).upper() != chr(adapter[j]))
        if d <= n // 10:
            return p
    return None


def passes(x: bytes) -> bool:
    return len(x) == 0 or len(x) > READ_MAX


def decide(a: bytes, b: Optional[bytes], s: Settings) -> List[Tuple[int, int]]:
    """Per mate (kept length, how): of a pair, or with ``b`` None of a single-end read."""
    mates = [a] + ([b] if b is not None else [])
    out = [(len(x), UNTOUCHED) for x in mates]
    if any(passes(x) for x in mates):
        return out
    if b is not None and s.overlap:
        inserts = accepted_inserts(a, b, s)
        if inserts:
            best = max(inserts)
            return [(min(len(x), best), BY_OVERLAP if best < len(x) else OVERLAP_CLEAN) for x in mates]
    for k, (x, adapter) in enumerate(zip(mates, (s.adapter_r1, s.adapter_r2))):
        p = adapter_position(x, adapter, s)
        if p is not None:
            out[k] = (p, BY_SEQUENCE)
    return out


class Trimmed(NamedTuple):
    """``reads``: per side the (bases, qualities) every record is left with; ``how``: per side; ``totals``: the six
    counts of gf_at_trim_device."""
    reads: List[List[Tuple[bytes, bytes]]]
    how: List[List[int]]
    totals: List[int]

    def counters(self) -> dict:
        return dict(zip(TOTAL_KEYS[1:], self.totals[1:]))


def trim_batch(left: Sequence[Tuple[bytes, bytes]], right: Optional[Sequence[Tuple[bytes, bytes]]] = None,
               s: Settings = Settings(), verdicts=None) -> Trimmed:
    """The trimming over records (bases, qualities) — with ``right`` their mates, record by record.  ``verdicts``: what
    ``decide`` gave for these records, when the caller has it already."""
    sides = [list(left)] + ([list(right)] if right is not None else [])
    assert all(len(x) == len(sides[0]) for x in sides)
    reads = [[] for _ in sides]
    how = [[] for _ in sides]
    totals = [0] * 6
    for i in range(len(sides[0])):
        verdict = verdicts[i] if verdicts is not None else \
            decide(sides[0][i][0], sides[1][i][0] if right is not None else None, s)
        if verdict[0][1] in (BY_OVERLAP, OVERLAP_CLEAN):
            totals[5] += 1
        for k, (kept, code) in enumerate(verdict):
            b, q = sides[k][i]
            totals[0] += 1
            if code in (BY_OVERLAP, BY_SEQUENCE):
                totals[1] += 1
                totals[2] += len(b) - kept
                totals[3 if code == BY_OVERLAP else 4] += 1
            reads[k].append((b[:kept], q[:kept]))
            how[k].append(code)
    return Trimmed(reads, how, totals)
