"""The definitions of include/gf_read_qc.h as plain loops over bytes, written from the header's text: what the host
program (tests/test_read_qc_core.py), the kernels and the routes (tests/test_read_qc_gpu.py) and the report
(tests/test_read_qc_plumbing.py) are held to.  No lanes, no rounds, no search order; the insert of a pair is
``max(accepted_inserts(a, b, Settings()))`` of tests/adapter_trim_model.py."""
import json
from typing import List, Optional, Sequence, Tuple

import numpy as np

from tests.adapter_trim_model import Settings, accepted_inserts

CYCLES = 512
SIDE_WORDS = 513 + 513 * 8
INSERT_WORDS = 1026
A, C, G, T, N, QUAL_SUM, Q20, Q30 = range(8)
LETTER = {"A": A, "C": C, "G": G, "T": T}


def phred(q: int) -> int:
    return max(q - 33, 0)


def stats_table(reads: Sequence[Tuple[bytes, bytes]], table: Optional[np.ndarray] = None) -> np.ndarray:
    """The records (bases, qualities) added into ``table`` (a new one of zeros without)."""
    table = np.zeros(SIDE_WORDS, dtype=np.int64) if table is None else table
    for b, q in reads:
        assert len(b) == len(q)
        table[min(len(b), CYCLES)] += 1
        for pos, (x, y) in enumerate(zip(b, q)):
            row = 513 + 8 * min(pos, CYCLES)
            table[row + LETTER.get(chr(x).upper(), N)] += 1
            table[row + QUAL_SUM] += phred(y)
            table[row + Q20] += phred(y) >= 20
            table[row + Q30] += phred(y) >= 30
    return table


def insert_entry(a: bytes, b: bytes) -> int:
    """The entry of the histogram the pair counts in."""
    if not (1 <= len(a) <= 512 and 1 <= len(b) <= 512):
        return 1025
    accepted = accepted_inserts(a, b, Settings())
    return max(accepted) if accepted else 0


def insert_hist(pairs: Sequence[Tuple[bytes, bytes]], hist: Optional[np.ndarray] = None) -> np.ndarray:
    hist = np.zeros(INSERT_WORDS, dtype=np.int64) if hist is None else hist
    for a, b in pairs:
        hist[insert_entry(a, b)] += 1
    return hist


def _rate(part: int, whole: int) -> float:
    return part / whole if whole else 0.0


def summary(tables: Sequence[np.ndarray]) -> dict:
    """The figures of one stage from its sides' tables."""
    reads, bases, q20, q30, gc = [], [], 0, 0, 0
    for t in tables:
        rows = [[int(x) for x in t[513 + 8 * c:513 + 8 * c + 8]] for c in range(513)]
        reads.append(sum(int(x) for x in t[1:513]))
        bases.append(sum(r[A] + r[C] + r[G] + r[T] + r[N] for r in rows))
        q20 += sum(r[Q20] for r in rows)
        q30 += sum(r[Q30] for r in rows)
        gc += sum(r[G] + r[C] for r in rows)
    out = {"total_reads": sum(reads), "total_bases": sum(bases), "q20_bases": q20, "q30_bases": q30,
           "q20_rate": _rate(q20, sum(bases)), "q30_rate": _rate(q30, sum(bases))}
    for k in range(len(tables)):
        out["read%d_mean_length" % (k + 1)] = bases[k] // reads[k] if reads[k] else 0
    out["gc_content"] = _rate(gc, sum(bases))
    return out


def curves(t: np.ndarray) -> dict:
    longest = max((L for L in range(1, 513) if t[L]), default=0)
    mean, content = [], {k: [] for k in ("A", "T", "C", "G", "N", "GC")}
    for c in range(min(longest, CYCLES)):
        r = [int(x) for x in t[513 + 8 * c:513 + 8 * c + 8]]
        n = r[A] + r[C] + r[G] + r[T] + r[N]
        mean.append(_rate(r[QUAL_SUM], n))
        for k, v in (("A", r[A]), ("T", r[T]), ("C", r[C]), ("G", r[G]), ("N", r[N]), ("GC", r[G] + r[C])):
            content[k].append(_rate(v, n))
    return {"total_cycles": longest, "quality_curves": {"mean": mean}, "content_curves": content}


def insert_size(hist: np.ndarray) -> dict:
    h = [int(x) for x in hist]
    peak, best, last = 0, 0, 0
    for i in range(30, 1025):
        if h[i] > best:   # (the smallest of equal counts stays)
            peak, best = i, h[i]
        if h[i]:
            last = i
    return {"peak": peak, "unknown": h[0] + h[1025], "histogram": h[:last + 1]}


def document(before: Sequence[np.ndarray], after: Sequence[np.ndarray], hist: Optional[np.ndarray] = None,
             counters: Optional[dict] = None) -> dict:
    doc = {"summary": {"before_filtering": summary(before), "after_filtering": summary(after)}}
    if counters is not None and "reads_passed" in counters:
        doc["filtering_result"] = {"passed_filter_reads": counters["reads_passed"],
                                   "low_quality_reads": counters["reads_low_quality"],
                                   "too_many_N_reads": counters["reads_too_many_n"],
                                   "too_short_reads": counters["reads_too_short"],
                                   "mate_failed_reads": counters["reads_mate_failed"]}
    if counters is not None and "adapter_reads_cut" in counters:
        doc["adapter_cutting"] = {"adapter_trimmed_reads": counters["adapter_reads_cut"],
                                  "adapter_trimmed_bases": counters["adapter_bases_cut"],
                                  "cut_by_overlap": counters["adapter_cut_by_overlap"],
                                  "cut_by_sequence": counters["adapter_cut_by_sequence"],
                                  "overlapping_pairs": counters["adapter_overlapping_pairs"]}
    if hist is not None:
        doc["insert_size"] = insert_size(hist)
    for stage, tables in (("before", before), ("after", after)):
        for k, t in enumerate(tables):
            doc["read%d_%s_filtering" % (k + 1, stage)] = curves(t)
    return doc


def report_json(before, after, hist=None, counters=None) -> str:
    return json.dumps(document(before, after, hist, counters), indent=1) + "\n"


def fastq_records(path: str) -> List[Tuple[bytes, bytes]]:
    """(bases, qualities) of every record of a FASTQ file; a final record needs no newline."""
    lines = open(path, "rb").read().split(b"\n")
    return [(lines[k + 1], lines[k + 3]) for k in range(0, len(lines) - 3, 4)]
