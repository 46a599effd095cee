"""The read filter's predicate (include/gf_read_filter.h) in plain Python, position by position: the statement that
gf_pp_core.h, the kernels of libgfprep.so and every route are held to.  Per read, per pair, and over a batch: the output
reads, the reasons and the eight totals."""
from typing import List, NamedTuple, Optional, Sequence, Tuple

MAX_READ_LEN = 4096
KEPT, TOO_SHORT, TOO_MANY_N, LOW_QUALITY, MATE_FAILED = 0, 1, 2, 3, 4
TOTAL_KEYS = ("reads", "reads_passed", "reads_trimmed", "bases_trimmed", "reads_too_short", "reads_too_many_n",
              "reads_low_quality", "reads_mate_failed")


class Settings(NamedTuple):
    poly_g_min: int = 10
    cut_tail_window: int = 0
    cut_tail_mean: int = 20
    length_required: int = 15
    n_base_limit: int = 5
    qualified_phred: int = 15
    unqualified_percent: int = 40


def phred(q: int) -> int:
    return max(q - 33, 0)


def decide(b: bytes, q: bytes, s: Settings = Settings()) -> Tuple[int, int]:
    """(kept length e2, the read's own reason).  ``q`` has the length of ``b``."""
    L = len(b)
    assert len(q) == L
    if L > MAX_READ_LEN:
        return L, KEPT
    e1 = L
    if s.poly_g_min > 0:
        t = 0
        while t < L and b[L - 1 - t] in b"Gg":
            t += 1
        if t >= s.poly_g_min:
            e1 = L - t
    e2 = e1
    W, M = s.cut_tail_window, s.cut_tail_mean
    if W > 0:
        e2 = 0
        for e in range(e1, W - 1, -1):
            if sum(phred(x) for x in q[e - W:e]) >= W * M:
                e2 = e
                break
    if e2 < s.length_required:
        return e2, TOO_SHORT
    if sum(1 for x in b[:e2] if x not in b"ACGTacgt") > s.n_base_limit:
        return e2, TOO_MANY_N
    low = sum(1 for x in q[:e2] if phred(x) < s.qualified_phred)
    if 100 * low > s.unqualified_percent * e2:
        return e2, LOW_QUALITY
    return e2, KEPT


class Filtered(NamedTuple):
    """``reads``: per side the (bases, qualities) every record is left with, b"" for a dropped one; ``reasons``: per
    side, after the pair rule; ``totals``: the eight counts of gf_pp_filter_device."""
    reads: List[List[Tuple[bytes, bytes]]]
    reasons: List[List[int]]
    totals: List[int]

    def counters(self) -> dict:
        return dict(zip(TOTAL_KEYS[1:], self.totals[1:]))


def filter_batch(left: Sequence[Tuple[bytes, bytes]], right: Optional[Sequence[Tuple[bytes, bytes]]] = None,
                 s: Settings = Settings()) -> Filtered:
    """The filter over records (bases, qualities) — with ``right`` their mates, record by record."""
    sides = [list(left)] + ([list(right)] if right is not None else [])
    assert all(len(x) == len(sides[0]) for x in sides)
    reads = [[] for _ in sides]
    reasons = [[] for _ in sides]
    totals = [0] * 8
    for i in range(len(sides[0])):
        own = [decide(*side[i], s) for side in sides]
        failed = any(r != KEPT for _, r in own)
        for k, (side, (e2, r)) in enumerate(zip(sides, own)):
            b, q = side[i]
            totals[0] += 1
            if r == KEPT and failed:
                r = MATE_FAILED
            if r == KEPT:
                totals[1] += 1
                if e2 < len(b):
                    totals[2] += 1
                    totals[3] += len(b) - e2
                reads[k].append((b[:e2], q[:e2]))
            else:
                totals[3 + r] += 1
                reads[k].append((b"", b""))
            reasons[k].append(r)
    return Filtered(reads, reasons, totals)
