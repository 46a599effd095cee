"""The predicate of include/gf_overlap_correct.h as plain loops over bytes, written from the header's text: what the
host program (tests/test_overlap_correct_core.py) and the kernel (tests/test_overlap_correct_gpu.py) are held to.  No
packing, no search order: I* is the largest of ``tests.adapter_trim_model.accepted_inserts``, and every position of the
overlap is looked at, one base at a time."""
from typing import List, NamedTuple, Optional, Sequence, Tuple

from tests.adapter_trim_model import Settings as TrimSettings
from tests.adapter_trim_model import accepted_inserts, complementary, passes

TOTAL_KEYS = ("pairs_seen", "correction_overlapping_pairs", "correction_pairs_with_diffs", "corrected_reads",
              "corrected_bases", "correction_diffs_left")
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}
LEFT, FIX_R1, FIX_R2 = 0, 1, 2


class Settings(NamedTuple):
    min_overlap: int = 30
    max_diff: int = 5
    diff_percent: int = 20
    good_phred: int = 30
    bad_phred: int = 15


def settings_error(s: Settings) -> bool:
    """Whether the library refuses ``s``."""
    return not (8 <= s.min_overlap <= 512 and 0 <= s.max_diff and 0 <= s.diff_percent <= 100
                and 0 <= s.good_phred <= 93 and 0 <= s.bad_phred <= 93 and s.bad_phred < s.good_phred)


def phred(q: int) -> int:
    return max(q - 33, 0)


def is_base(x: int) -> bool:
    return chr(x).upper() in COMPLEMENT


def decide(a: int, qa: int, b: int, qb: int, s: Settings) -> int:
    """One difference: which mate is rewritten."""
    if is_base(a) and phred(qa) >= s.good_phred and phred(qb) <= s.bad_phred:
        return FIX_R2
    if is_base(b) and phred(qb) >= s.good_phred and phred(qa) <= s.bad_phred:
        return FIX_R1
    return LEFT


def insert_of(a: bytes, b: bytes, s: Settings) -> int:
    """I*, -1 without one."""
    if passes(a) or passes(b):
        return -1
    got = accepted_inserts(a, b, TrimSettings(min_overlap=s.min_overlap, max_diff=s.max_diff,
                                              diff_percent=s.diff_percent))
    return max(got) if got else -1


class Corrected(NamedTuple):
    a: bytes
    qa: bytes
    b: bytes
    qb: bytes
    insert: int
    fixed: Tuple[int, int]   # bases corrected in R1, in R2
    left: int                # differences left standing
    branches: Tuple[str, ...] = ()   # what happened at each difference, in the order of i


def correct_pair(a: bytes, qa: bytes, b: bytes, qb: bytes, s: Settings = Settings()) -> Corrected:
    insert = insert_of(a, b, s)
    if insert < 0:
        return Corrected(a, qa, b, qb, -1, (0, 0), 0)
    xa, xqa, xb, xqb = bytearray(a), bytearray(qa), bytearray(b), bytearray(qb)
    lo, hi = max(0, insert - len(b)), min(insert, len(a))
    fixed, left, branches = [0, 0], 0, []
    for i in range(lo, hi):
        j = insert - 1 - i
        if complementary(a[i], b[j]):
            continue
        what = decide(a[i], qa[i], b[j], qb[j], s)
        if what == FIX_R2:
            xb[j], xqb[j] = ord(COMPLEMENT[chr(a[i]).upper()]), qa[i]
            fixed[1] += 1
            branches.append("r2")
        elif what == FIX_R1:
            xa[i], xqa[i] = ord(COMPLEMENT[chr(b[j]).upper()]), qb[j]
            fixed[0] += 1
            branches.append("r1")
        else:
            left += 1
            branches.append("left")
    return Corrected(bytes(xa), bytes(xqa), bytes(xb), bytes(xqb), insert, (fixed[0], fixed[1]), left, tuple(branches))


class Batch(NamedTuple):
    """``reads``: per side the (bases, qualities) every record is left with; ``insert``: per pair; ``fixed``: R1's, then
    R2's; ``totals``: the six counts of gf_oc_correct_device."""
    reads: List[List[Tuple[bytes, bytes]]]
    insert: List[int]
    fixed: List[int]
    totals: List[int]

    def counters(self) -> dict:
        return dict(zip(TOTAL_KEYS[1:], self.totals[1:]))


def correct_batch(left: Sequence[Tuple[bytes, bytes]], right: Sequence[Tuple[bytes, bytes]],
                  s: Settings = Settings(), answers: Optional[Sequence[Corrected]] = None) -> Batch:
    """The correction over pairs of records (bases, qualities).  ``answers``: what ``correct_pair`` gave for these
    pairs, when the caller has it already."""
    assert len(left) == len(right)
    reads, inserts, fixed_l, fixed_r, totals = [[], []], [], [], [], [0] * 6
    for k, ((a, qa), (b, qb)) in enumerate(zip(left, right)):
        c = answers[k] if answers is not None else correct_pair(a, qa, b, qb, s)
        reads[0].append((c.a, c.qa))
        reads[1].append((c.b, c.qb))
        inserts.append(c.insert)
        fixed_l.append(c.fixed[0])
        fixed_r.append(c.fixed[1])
        totals[0] += 1
        totals[1] += c.insert >= 0
        totals[2] += sum(c.fixed) + c.left > 0
        totals[3] += (c.fixed[0] > 0) + (c.fixed[1] > 0)
        totals[4] += sum(c.fixed)
        totals[5] += c.left
    return Batch(reads, inserts, fixed_l + fixed_r, totals)
