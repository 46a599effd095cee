"""The five read-preparation libraries past one tile per thread of their offsets scan: the read filter (libgfprep.so),
adapter trimming (libgfadapt.so), the UMI cut (libgfumi.so), duplicate removal (libgfdedup.so) and the FASTQ writer
(libgfwrite.so).  Each ends in the same three stages: a per-tile kernel leaves tile-relative offsets and one sum per tile
and side; gf_pp_k_scan<1> or gf_pp_k_scan<2> (gf_pp_kernels.h over gf_scan_totals_block, gf_scan_common.h) scans the
tile sums with ONE block of SCAN_THREADS threads, thread t taking a run of ``per = ceil(tiles / SCAN_THREADS)`` sums;
gf_pp_k_gather or gf_rw_k_format makes the offsets absolute and moves the bytes.  Every library has a workspace layout
and a launch of the scan of its own.  A tile is PP_TILE records, so ``per = 1`` holds up to 262 144 records, and a chunk
of a real run is about a million pairs: the other modules stay at a few hundred records, these batches are the smallest
that cross each threshold (SHAPES).

Every record, or pair, is drawn from a pool of at most POOL_MAX distinct entries of at most about LEN_MAX bases, built
from the edge cases the libraries' own tests have; the Python model runs once per pool entry, a seeded sequence says which
entry every record is, and lengths, codes, totals, offsets and bytes follow from the sequence by numpy gathers and one
``b"".join``.  Without a GPU the module holds its constants to the sources, its shapes to the thresholds, and its inputs
to the condition that keeps the device tests from passing over a wrong scan: a numpy statement of the two-level scan
that takes a fault gives other tile starts, for every library and every shape past the threshold, than the expected
output was built from.

Every device case runs twice: through the function the library's other tests use, and through the same library's ctypes
entry point with exactly ``*_workspace_bytes(n)`` bytes of workspace inside sentinels (the functions allocate the
workspace themselves), the outputs inside sentinels too."""
import ctypes as C
import functools
import os
import re
from typing import NamedTuple, Tuple

import numpy as np
import pytest

from tests import adapter_trim_cases as at_cases
from tests import adapter_trim_model as at_model
from tests import read_filter_cases as rf_cases
from tests import read_filter_model as rf_model
from tests import read_write_cases as rw_cases
from tests import read_write_model as rw_model
from tests import umi_cases, umi_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN_CSRC = os.path.join(ROOT, "genefuserust_amd", "scan_csrc")

WAVE = 64                           # lanes of a wavefront
BLOCK = 256                         # GF_SCAN_THREADS: the per-tile kernels' block
SCAN_THREADS = 1024                 # GF_SCAN_TOTALS_THREADS: the one block that scans the tile sums
PP_TILE = BLOCK                     # GF_PP_TILE: records per tile

# the smallest batches that cross each threshold (scan_shape says what each is)
SHAPES = {
    "A": WAVE * PP_TILE + PP_TILE + 5,                          # the second wavefront of the scan block, a partial tile
    "B": SCAN_THREADS * PP_TILE,                                # every thread a run of one, a whole last tile
    "C": SCAN_THREADS * PP_TILE + 1,                            # runs of two, the last run of one, one record in it
    "D": (SCAN_THREADS + SCAN_THREADS // 2) * PP_TILE + 131,    # runs of two, threads left over, a partial tile
    "E": 2 * SCAN_THREADS * PP_TILE + 1,                        # runs of three, the last run whole, one record in it
}
PAST = ("C", "D", "E")              # per >= 2
LIBRARIES = ("filter", "adapter", "umi", "dedup", "writer")
SOURCE_FILES = {"filter": "gf_read_filter.hip", "adapter": "gf_adapter_trim.hip", "umi": "gf_umi.hip",
                "dedup": "gf_dedup.hip", "writer": "gf_read_write.hip"}

POOL_MAX, LEN_MAX = 256, 40
LEADS = (3, 9)                      # where the first byte of each side lies behind a 16-byte boundary
GUARD, FILL, WS_FILL, OFF_FILL = 64, 0xEE, 0x11, -77
WS_WORD = int.from_bytes(bytes([WS_FILL]) * 8, "little")   # what an int64 read from the sentinels around a workspace gives
FIRST_INDEX = (1 << 40) + 7
DEDUP_SLOTS = 1 << 20
UMI_LENGTH, UMI_SKIP = 8, 2
FAULTS = ("per1", "no_wave_base", "sides_swapped", "short_last_run", "second_sequence_base_of_first")


def scan_shape(n: int) -> Tuple[int, int, int, int]:
    """(tiles, per, threads that have a run, length of the last run) of the one-block scan over the tile sums of n
    records."""
    tiles = -(-n // PP_TILE)
    per = max(-(-tiles // SCAN_THREADS), 1)
    busy = -(-tiles // per)
    return tiles, per, busy, tiles - (busy - 1) * per


# ---- 0. the sizes are the sources' -----------------------------------------------------------------------------------

def _source(name: str) -> str:
    with open(os.path.join(SCAN_CSRC, name)) as f:
        return f.read()


def _define(header: str, name: str) -> str:
    m = re.search(r"^#define\s+%s\s+(.+?)\s*(?://.*)?$" % name, _source(header), flags=re.M)
    assert m, (header, name)
    return m.group(1)


def test_sizes_are_the_sources():
    assert int(_define("gf_scan_common.h", "GF_SCAN_THREADS")) == BLOCK
    assert int(_define("gf_scan_common.h", "GF_SCAN_TOTALS_THREADS")) == SCAN_THREADS
    assert _define("gf_pp_kernels.h", "GF_PP_TILE") == "GF_SCAN_THREADS"
    # the split into runs is written once, in the shared body, and the scan kernel is one block of the totals' threads
    split = r"per = \((?:ntiles|n) \+ GF_SCAN_TOTALS_THREADS - 1\) / GF_SCAN_TOTALS_THREADS;"
    assert len(re.findall(split, _source("gf_scan_common.h"))) == 1
    pp = _source("gf_pp_kernels.h")
    assert not re.findall(split, pp)
    assert len(re.findall(r"__launch_bounds__\(GF_SCAN_TOTALS_THREADS\)\s+void gf_pp_k_scan\(", pp)) == 1
    for library, name in SOURCE_FILES.items():
        src = _source(name)
        assert re.findall(r"\.tiles = (.+?);", src) == ["(n + GF_PP_TILE - 1) / GF_PP_TILE"], library
        for s in (1, 2):
            launch = r"hipLaunchKernelGGL\(gf_pp_k_scan<%d>,\s*dim3\((\w+)\),\s*dim3\((\w+)\),\s*0,\s*st,\s*sum_l,\s*sum_r,\s*" \
                     r"W\.tiles,\s*n," % s
            assert re.findall(launch, src) == [("1", "GF_SCAN_TOTALS_THREADS")], (library, s)


def test_shapes_cross_the_thresholds():
    want = {"A": (66, 1, 66, 1), "B": (1024, 1, 1024, 1), "C": (1025, 2, 513, 1), "D": (1537, 2, 769, 1),
            "E": (2049, 3, 683, 3)}
    assert {k: scan_shape(n) for k, n in SHAPES.items()} == want
    tiles, per, busy, _ = scan_shape(SHAPES["A"])
    assert per == 1 and WAVE < busy <= 2 * WAVE and SHAPES["A"] % PP_TILE == 5     # the second wavefront, a partial tile
    assert scan_shape(SHAPES["B"])[1:3] == (1, SCAN_THREADS) and SHAPES["B"] % PP_TILE == 0
    assert SHAPES["C"] == SHAPES["B"] + 1                                          # one record past per = 1
    for k in PAST:
        tiles, per, busy, last = scan_shape(SHAPES[k])
        assert per >= 2 and busy < SCAN_THREADS and SHAPES[k] % PP_TILE != 0
    assert scan_shape(SHAPES["C"])[3] < scan_shape(SHAPES["C"])[1] and scan_shape(SHAPES["D"])[3] < scan_shape(SHAPES["D"])[1]
    assert SHAPES["C"] % PP_TILE == 1 == SHAPES["E"] % PP_TILE and SHAPES["D"] % PP_TILE == 131


# ---- 1. the two-level scan, in numpy, with a fault -----------------------------------------------------------------------

def two_level_scan(sums: np.ndarray, fault: str = None, behind: int = WS_WORD) -> np.ndarray:
    """gf_pp_k_scan over ``sums`` (int64[S, tiles]; S = 1 or 2 sequences), as gf_scan_totals_block does it: thread t of
    SCAN_THREADS takes the run [t per, t per + per) cut at ``tiles``, the runs' sums are scanned inside each wavefront,
    a wavefront's base is the sum of the wavefronts in front of it, and an element's offset is its run's base plus its
    place in the run; in place, entry ``tiles`` the sum.  Returns int64[S, tiles + 1].  ``behind``: what the memory behind
    the sums reads as.  ``fault``: one of FAULTS —

      per1                            runs of one: the tiles past SCAN_THREADS stay as they were
      no_wave_base                    the base of the wavefronts 1 and up dropped
      sides_swapped                   sequence 0's result where sequence 1's belongs, and the reverse
      short_last_run                  a run is not cut at ``tiles``: the last one reads past the sums
      second_sequence_base_of_first   sequence 1 placed with sequence 0's wavefront bases"""
    assert fault is None or fault in FAULTS
    S, tiles = sums.shape
    per = 1 if fault == "per1" else max(-(-tiles // SCAN_THREADS), 1)
    mem = np.full((S, max(SCAN_THREADS * per, tiles) + per + 1), behind, dtype=np.int64)
    mem[:, :tiles] = sums
    t0 = np.minimum(np.arange(SCAN_THREADS, dtype=np.int64) * per, tiles)
    t1 = t0 + per if fault == "short_last_run" else np.minimum(t0 + per, tiles)
    idx = t0[:, None] + np.arange(per, dtype=np.int64)[None, :]
    mine_of = idx < t1[:, None]
    with np.errstate(over="ignore"):
        vals = np.where(mine_of[None], mem[:, idx], 0)                         # [S, thread, place in the run]
        mine = vals.sum(axis=2).reshape(S, SCAN_THREADS // WAVE, WAVE)
        y = np.cumsum(mine, axis=2)                                            # inclusive, inside a wavefront
        wave_sum = y[:, :, -1]
        base = np.cumsum(wave_sum, axis=1) - wave_sum                          # the wavefronts in front
        total = wave_sum.sum(axis=1)
        if fault == "no_wave_base":
            base = np.zeros_like(base)
        if fault == "second_sequence_base_of_first" and S == 2:
            base = np.stack([base[0], base[0]])
        pos = (base[:, :, None] + y - mine).reshape(S, SCAN_THREADS)
        at = pos[:, :, None] + np.cumsum(vals, axis=2) - vals
    out = mem.copy()
    for s in range(S):
        out[s][idx[mine_of]] = at[s][mine_of]
    out[:, tiles] = total
    if fault == "sides_swapped" and S == 2:
        out = out[::-1]
    return out[:, :tiles + 1].copy()


def test_the_statement_is_an_exclusive_scan():
    rng = np.random.default_rng(4)
    for tiles in (1, WAVE, WAVE + 1, SCAN_THREADS, SCAN_THREADS + 1, 2 * SCAN_THREADS + 2, 3 * SCAN_THREADS + 1):
        for S in (1, 2):
            sums = rng.integers(0, 5000, (S, tiles))
            want = np.concatenate([np.zeros((S, 1), np.int64), np.cumsum(sums, axis=1)], axis=1)
            assert np.array_equal(two_level_scan(sums), want)


# ---- 2. pools: the model once per entry ----------------------------------------------------------------------------------

class Pool(NamedTuple):
    """K entries.  ``ins`` / ``outs``: per side, per entry, what goes in and what the model leaves — (bases, qualities),
    for the writer's ``outs`` the FASTQ text.  ``codes``: the columns of per-record codes the call leaves (reasons, how
    flags, UMI codes), per entry.  ``totals``: int64[K, counters], what one record of the entry adds.  ``more``: what only
    one library has."""
    ins: tuple
    outs: tuple
    codes: tuple
    totals: np.ndarray
    more: dict

    @property
    def sides(self) -> int:
        return len(self.ins)

    def kept(self) -> np.ndarray:
        """int64[sides, K]: the bytes an entry leaves on each side."""
        return np.array([[len(o if isinstance(o, bytes) else o[0]) for o in side] for side in self.outs], dtype=np.int64)

    def had(self) -> np.ndarray:
        return np.array([[len(x if isinstance(x, bytes) else x[0]) for x in side] for side in self.ins], dtype=np.int64)


def _distinct(items, limit=POOL_MAX):
    return list(dict.fromkeys(items))[:limit]


FILTER_SETTINGS = rf_model.Settings(poly_g_min=4, cut_tail_window=4, cut_tail_mean=20, length_required=8, n_base_limit=2,
                                    qualified_phred=15, unqualified_percent=60)


@functools.lru_cache(maxsize=None)
def filter_pool(sides: int) -> Pool:
    """The read filter's edge reads of at most LEN_MAX bases at small settings, and random ones; a pair is a read and the
    read 37 further on."""
    s = FILTER_SETTINGS
    rng = np.random.default_rng(40)
    clean = [(rf_cases.bases_of(rng, int(L)), bytes([rf_cases.GOOD]) * int(L)) for L in rng.integers(8, LEN_MAX + 1, 170)]
    reads = _distinct([r for r in rf_cases.edge_reads(s) + rf_cases.random_reads(500, 41, longest=LEN_MAX)
                       if len(r[0]) <= LEN_MAX][:POOL_MAX - len(clean)] + clean)
    ins = [reads] + ([reads[37:] + reads[:37]] if sides == 2 else [])
    outs, reasons, totals = [[] for _ in ins], [[] for _ in ins], []
    for k in range(len(reads)):
        m = rf_model.filter_batch([ins[0][k]], [ins[1][k]] if sides == 2 else None, s)
        for side in range(sides):
            outs[side].append(m.reads[side][0])
            reasons[side].append(m.reasons[side][0])
        totals.append(m.totals)
    return Pool(tuple(ins), tuple(outs), tuple(np.array(r, dtype=np.uint8) for r in reasons),
                np.array(totals, dtype=np.int64), {})


@functools.lru_cache(maxsize=None)
def adapter_pool(sides: int) -> Pool:
    """The adapter trimming's cases of at most LEN_MAX bases at the "smallest" settings (an adapter of four bases on R1,
    of 64 on R2, an overlap of eight with no difference), and random read-through pairs of that size; single-end: the
    sequence step's reads."""
    s = at_cases.SETTINGS["smallest"]
    rng = np.random.default_rng(52)
    rb = lambda n: at_cases.bases_of(rng, n)   # noqa: E731
    if sides == 2:
        planted = [(b"", b""), (b"ACGT" + rb(20), rb(33)), (rb(31), s.adapter_r2[:30]), (b"ACGT" + rb(9), s.adapter_r2[:25]),
                   (rb(40), b""), (b"", rb(17))]
        items = planted + [p for p in at_cases.pair_cases("smallest") if max(len(p[0]), len(p[1])) <= LEN_MAX]
        items = _distinct(items + [(rb(int(a)), rb(int(b))) for a, b in rng.integers(1, LEN_MAX + 1, (60, 2))]
                          + at_cases.random_pairs(400, 23, s, LEN_MAX))
        ins = [[(a, at_cases.quals_of(a)) for a, _ in items], [(b, at_cases.quals_of(b)) for _, b in items]]
    else:
        items = [r for r in at_cases.single_cases("smallest") if len(r) <= LEN_MAX]
        for L in rng.integers(13, LEN_MAX + 1, 300).tolist():
            r, p = rb(L), int(rng.integers(0, L))
            items.append(r if p % 2 else (r[:p] + b"ACGT" + r[p:])[:L])
        items = _distinct(items)
        ins = [[(a, at_cases.quals_of(a)) for a in items]]
    outs, how, totals = [[] for _ in ins], [[] for _ in ins], []
    for k in range(len(items)):
        verdict = at_model.decide(ins[0][k][0], ins[1][k][0] if sides == 2 else None, s)
        m = at_model.trim_batch([ins[0][k]], [ins[1][k]] if sides == 2 else None, s, [verdict])
        for side in range(sides):
            outs[side].append(m.reads[side][0])
            how[side].append(m.how[side][0])
        totals.append(m.totals)
    return Pool(tuple(ins), tuple(outs), tuple(np.array(h, dtype=np.uint8) for h in how), np.array(totals, dtype=np.int64),
                {"settings": s})


@functools.lru_cache(maxsize=None)
def _short_records(sides: int):
    """Reads or pairs whose lengths walk through the lengths around a UMI of 8 bases and a spacer of 2, the mates out of
    step: every combination of a side too short for the UMI, a side of exactly its length and a longer one occurs."""
    rng = np.random.default_rng(61)
    c = UMI_LENGTH + UMI_SKIP
    lens = [0, c - 1, c, c + 1, 15, 16, 17, 30, LEN_MAX]
    out = []
    for i in range(180):
        a = umi_cases.record(rng, lens[i % len(lens)])
        out.append((a, umi_cases.record(rng, lens[(i // len(lens) + 3 * i) % len(lens)])) if sides == 2 else a)
    return out


@functools.lru_cache(maxsize=None)
def umi_pool(sides: int, source: str) -> Pool:
    recs = _short_records(sides)
    ins = [[r[s] for r in recs] for s in (0, 1)] if sides == 2 else [list(recs)]
    outs, codes, totals = [[] for _ in ins], [], []
    for rec in recs:
        m = umi_model.cut(umi_model.SOURCES[source], UMI_LENGTH, UMI_SKIP, [rec])
        left = m.records[0] if sides == 2 else (m.records[0],)
        for side in range(sides):
            outs[side].append(left[side])
        codes.append(m.codes[0])
        totals.append(m.totals)
    return Pool(tuple(ins), tuple(outs), (np.array(codes, dtype=np.uint64),), np.array(totals, dtype=np.int64), {})


@functools.lru_cache(maxsize=None)
def dedup_pool(sides: int) -> Pool:
    """The same records; what a record leaves when it is no duplicate is the record."""
    recs = _short_records(sides)
    ins = [[r[s] for r in recs] for s in (0, 1)] if sides == 2 else [list(recs)]
    return Pool(tuple(ins), tuple(ins), (), np.zeros((len(recs), 0), dtype=np.int64), {})


WRITER_NAME_LENGTHS = [2, 5, 9, 15, 16, 17, 23, 30]
WRITER_KEPT = {1: ([0, 1, 15, 0, 16, 17, 0, 25, 30],), 2: ([0, 1, 15, 16, 0, 17, 25, 30, 28], [0, 14, 16, 31, 2, 29])}


@functools.lru_cache(maxsize=None)
def writer_pool(sides: int, tagged: bool) -> Pool:
    """Records as tests/read_write_cases.py's ``build`` makes them, under names of 2 to 30 bytes with colons, a third
    with a space and a comment, a third with a tab: per entry and side the FASTQ text of the record as the sequencer
    wrote it, the record ahead of the UMI cut, the record as the steps left it (about a third of the entries have a
    mate without bases), and from the model the text that is written."""
    rng = np.random.default_rng(71)
    source, length = (rw_model.PER_READ, UMI_LENGTH) if tagged else (rw_model.NAME, 0)
    c = UMI_LENGTH + UMI_SKIP if tagged else 0
    texts, pre, finals, outs = ([[] for _ in range(sides)] for _ in range(4))
    totals = []
    for i in range(180):
        for s in range(sides):
            kept = WRITER_KEPT[sides][s]
            keep = kept[i % len(kept)] if s == 0 else kept[(i // len(kept) + 3 * i) % len(kept)]
            total = c + keep + (i + s) % 3
            b, q = umi_cases.random_bases(rng, total), umi_cases.random_quals(rng, total)
            name = rw_cases.name_line(rng, WRITER_NAME_LENGTHS[(i + 3 * s) % len(WRITER_NAME_LENGTHS)],
                                      (i // len(WRITER_NAME_LENGTHS) + s) % 3)
            texts[s].append(umi_cases.fastq_text([name], [(b, q)]))
            pre[s].append((b, q))
            finals[s].append((b[c:c + keep], q[c:c + keep]))
        m = rw_model.format_reads([t[i] for t in texts], [[f[i]] for f in finals], source, length, [[p[i]] for p in pre])
        for s in range(sides):
            outs[s].append(m.texts[s])
        totals.append(m.totals)
    return Pool(tuple(texts), tuple(outs), (), np.array(totals, dtype=np.int64),
                {"finals": tuple(finals), "pre": tuple(pre), "source": source, "length": length})


def pool_of(library: str, sides: int) -> Pool:
    return {"filter": lambda: filter_pool(sides), "adapter": lambda: adapter_pool(sides),
            "umi": lambda: umi_pool(sides, "per_read" if sides == 2 else "read1"), "dedup": lambda: dedup_pool(sides),
            "writer": lambda: writer_pool(sides, True)}[library]()


def test_pools_hold_every_kind():
    for library in LIBRARIES:
        for sides in (1, 2):
            pool = pool_of(library, sides)
            K = len(pool.ins[0])
            assert 100 <= K <= POOL_MAX and all(len(x) == K for x in pool.ins + pool.outs), (library, sides)
            if library != "writer":
                assert pool.had().max() <= LEN_MAX + 1 and len(set(zip(*pool.ins))) > 0.8 * K
    # pairs: the sides keep different lengths in most entries; entries that keep nothing on one side, nothing on either
    # and everything.  (The read filter drops a pair as a whole: there a side keeps nothing only with its mate.  The
    # removal keeps a record or drops it, so its kinds are those of the records themselves.)
    for library in LIBRARIES:
        pool = pool_of(library, 2)
        kept, had = pool.kept(), pool.had()
        assert (kept[0] != kept[1]).mean() > 0.5, library
        if library != "dedup":
            assert ((kept[0] == 0) & (kept[1] == 0) & (had[0] + had[1] > 0)).any(), library
        if library == "writer":   # (both mates are written or neither: the mate without bases is in what goes in)
            left = np.array([[len(f[0]) for f in side] for side in pool.more["finals"]])
            assert ((left[0] == 0) & (left[1] > 0)).any() and ((left[0] > 0) & (left[1] == 0)).any()
        elif library != "filter":
            assert ((kept[0] == 0) & (kept[1] > 0)).any() and ((kept[0] > 0) & (kept[1] == 0)).any(), library
        if library not in ("writer", "umi"):   # (the text is longer than the record; the cut takes the UMI off a kept one)
            assert ((kept == had).all(axis=0) & (had > 0).all(axis=0)).any(), library
    whole = umi_pool(2, "read1")
    assert ((whole.kept()[1] == whole.had()[1]) & (whole.kept()[0] > 0)).any()              # R2 whole behind a cut R1
    f = filter_pool(2)
    assert {int(r) for col in f.codes for r in col} == {rf_model.KEPT, rf_model.TOO_SHORT, rf_model.TOO_MANY_N,
                                                        rf_model.LOW_QUALITY, rf_model.MATE_FAILED}
    assert (f.totals[:, 2] > 0).any()                                                  # trimmed and kept
    a = adapter_pool(2)
    assert {int(h) for col in a.codes for h in col} == {at_model.UNTOUCHED, at_model.BY_OVERLAP, at_model.BY_SEQUENCE,
                                                        at_model.OVERLAP_CLEAN}
    assert set(adapter_pool(1).codes[0].tolist()) == {at_model.UNTOUCHED, at_model.BY_SEQUENCE}
    for source in ("read1", "read2", "per_read"):
        u = umi_pool(2, source)
        assert (u.codes[0] == 0).any() and (u.totals[:, 5] > 0).any() and (u.totals[:, 3] > 0).any()   # too short; an N
        short = [k for k in range(len(u.codes[0])) if u.codes[0][k] == 0]
        assert any(len(u.ins[0][k][0]) > 0 for k in short) and any(len(u.ins[1][k][0]) > 0 for k in short)
    for sides in (1, 2):
        for tagged in (False, True):
            w = writer_pool(sides, tagged)
            dropped = w.totals[:, 4].mean()
            assert 0.25 < dropped < 0.45, (sides, tagged, dropped)                    # about a third is not written
            names = [t.split(b"\n")[0] for side in w.ins for t in side]
            assert {len(x) for x in names} == set(WRITER_NAME_LENGTHS)
            assert any(b" " in x for x in names) and any(b"\t" in x for x in names) and any(b":" in x for x in names)
    tagged = writer_pool(2, True)
    k = int(np.flatnonzero(tagged.totals[:, 0])[0])
    tag = rw_model.tag(rw_model.PER_READ, UMI_LENGTH, [tagged.more["pre"][s][k][0] for s in (0, 1)])
    assert len(tag) == 2 * UMI_LENGTH + 2 and all(tag in tagged.outs[s][k].split(b"\n")[0] for s in (0, 1))


# ---- 3. a batch from a pool -------------------------------------------------------------------------------------------------

class Plan(NamedTuple):
    """A batch of n records: ``seq[i]`` the pool entry of record i, ``live[i]`` 0 for a record that leaves nothing whatever
    its entry does (a duplicate); what follows from them without touching a byte: the bytes every record leaves per side,
    the offsets of the output, the tile sums the per-tile kernel has to leave, the totals."""
    n: int
    seq: np.ndarray
    live: np.ndarray
    kept: np.ndarray          # int64[sides, n]
    out_off: np.ndarray       # int64[sides, n + 1]
    tile_sums: np.ndarray     # int64[sides, tiles]
    totals: np.ndarray


def plan_of(pool: Pool, n: int, seed: int, duplicates: bool = False) -> Plan:
    rng = np.random.default_rng(seed)
    seq = rng.integers(0, len(pool.ins[0]), n)
    live = np.ones(n, dtype=np.int64)
    if duplicates:   # p = 0.5; a record without bases has no key and is none
        live = 1 - ((rng.random(n) < 0.5) & (pool.had().sum(axis=0)[seq] > 0)).astype(np.int64)
    kept = pool.kept()[:, seq] * live
    out_off = np.concatenate([np.zeros((pool.sides, 1), np.int64), np.cumsum(kept, axis=1)], axis=1)
    tile_sums = np.add.reduceat(kept, np.arange(0, n, PP_TILE), axis=1)
    totals = np.bincount(seq, minlength=len(pool.ins[0])) @ pool.totals
    return Plan(n, seq, live, kept, out_off, tile_sums, totals)


def library_plan(library: str, sides: int, shape: str) -> Tuple[Pool, Plan]:
    pool = pool_of(library, sides)
    return pool, plan_of(pool, SHAPES[shape], seed=sum(shape.encode()) + sides, duplicates=library == "dedup")


def _joined(entries, seq: np.ndarray, live: np.ndarray = None) -> bytes:
    """The entries of the records, one after the other; a record that is not ``live`` gives nothing."""
    picked = map(entries.__getitem__, seq.tolist())
    if live is None:
        return b"".join(picked)
    return b"".join(e for e, on in zip(picked, live.tolist()) if on)


def test_plans_follow_from_the_sequence():
    """A plan against the model over every record of a batch of three tiles: the one place where the model runs per
    record."""
    n = 2 * PP_TILE + 77
    for sides in (1, 2):
        pool = filter_pool(sides)
        plan = plan_of(pool, n, seed=9)
        reads = [[side[k] for k in plan.seq] for side in pool.ins]
        m = rf_model.filter_batch(reads[0], reads[1] if sides == 2 else None, FILTER_SETTINGS)
        assert plan.totals.tolist() == m.totals
        for s in range(sides):
            assert plan.kept[s].tolist() == [len(r[0]) for r in m.reads[s]]
            assert _joined([o[0] for o in pool.outs[s]], plan.seq) == b"".join(r[0] for r in m.reads[s])
            assert pool.codes[s][plan.seq].tolist() == m.reasons[s]
        pool = writer_pool(sides, True)
        plan = plan_of(pool, n, seed=9)
        m = rw_model.format_reads([_joined(side, plan.seq) for side in pool.ins],
                                  [[side[k] for k in plan.seq] for side in pool.more["finals"]], pool.more["source"],
                                  pool.more["length"], [[side[k] for k in plan.seq] for side in pool.more["pre"]])
        assert plan.totals.tolist() == m.totals and plan.out_off.tolist() == m.offsets
        assert [_joined(side, plan.seq) for side in pool.outs] == m.texts


@pytest.mark.parametrize("shape", PAST)
@pytest.mark.parametrize("library", LIBRARIES)
def test_a_wrong_scan_changes_a_tile_start(library, shape):
    """From the tile sums the device test expects (never from the device): the faultless statement gives the offsets
    the expected output is built from, and each fault another start of at least one tile on the side it touches — entry
    ``tiles``, where a tile behind the last would start, counts: it is the end of the last tile's bytes and the last
    offset.  short_last_run shows there alone, and only when the memory behind the sums does not read as 0: the device
    tests lay the workspace into WS_FILL bytes, which is what the statement reads there."""
    pool, plan = library_plan(library, 2, shape)
    tiles, per, busy, last = scan_shape(plan.n)
    assert plan.tile_sums.shape == (2, tiles) and per >= 2
    right = two_level_scan(plan.tile_sums)
    for s in (0, 1):
        assert np.array_equal(right[s][:tiles], plan.out_off[s][0:plan.n:PP_TILE]) and right[s][tiles] == plan.out_off[s][-1]
        # tile sums that are not all alike, past SCAN_THREADS too
        assert len(set(plan.tile_sums[s][SCAN_THREADS:].tolist())) > 1 or tiles - SCAN_THREADS == 1
    for fault in FAULTS:
        wrong = two_level_scan(plan.tile_sums, fault)
        touched = (1,) if fault == "second_sequence_base_of_first" else (0, 1)
        for s in touched:
            assert (wrong[s] != right[s]).any(), (fault, s)
        if fault == "short_last_run":
            assert all((wrong[s][:tiles] == right[s][:tiles]).all() and wrong[s][tiles] != right[s][tiles] for s in (0, 1))
    single_pool, single = library_plan(library, 1, shape)
    right = two_level_scan(single.tile_sums)
    assert np.array_equal(right[0][:tiles], single.out_off[0][0:single.n:PP_TILE])
    for fault in ("per1", "no_wave_base", "short_last_run"):
        assert (two_level_scan(single.tile_sums, fault) != right).any(), fault


# ---- 4. on the device ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ix(gpu_device):
    from genefuserust_amd import Indexer
    index = Indexer.from_gene_slices([b"ACGT" * 64])
    index.make_index()
    yield index
    index.close()


def _up(x: bytes):
    import torch
    return torch.from_numpy(np.frombuffer(x, dtype=np.uint8).copy()).cuda()


def _records_batch(entries, plan: Plan, lead: int):
    """The records of a plan as the full FASTQ cut leaves them, ``lead`` bytes of another record in front of the first."""
    import torch
    from genefuserust_amd.fastq import FastqBatch
    lens = np.array([len(e[0]) for e in entries], dtype=np.int64)[plan.seq]
    off = lead + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    none = torch.zeros(0, dtype=torch.int64, device="cuda")
    return FastqBatch(_up(b"G" * lead + _joined([e[0] for e in entries], plan.seq)),
                      _up(b"~" * lead + _joined([e[1] for e in entries], plan.seq)), torch.from_numpy(off).cuda(), plan.n,
                      none, 0, 0)


def _same_bytes(got, want: bytes, what):
    g = got.cpu().numpy()
    w = np.frombuffer(want, dtype=np.uint8)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, int(bad[0]), int(g[bad[0]]), int(w[bad[0]]))


def _same_array(got, want: np.ndarray, what):
    g = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    if want.dtype == np.uint64:
        g = g.view(np.uint64)
    assert g.shape == want.shape, (what, g.shape, want.shape)
    bad = np.flatnonzero(g != want)
    assert bad.size == 0, (what, int(bad[0]), int(g[bad[0]]), int(want[bad[0]]))


class Sentinelled(NamedTuple):
    whole: object     # the tensor, FILL all over before the call
    first: int        # where the part the library is given starts
    size: int         # how long that part is

    def ptr(self) -> int:
        return self.whole.data_ptr() + self.first

    def part(self, used: int):
        """The first ``used`` bytes of the library's part, after the check that nothing else was touched."""
        assert bool((self.whole[:self.first] == FILL).all()) and bool((self.whole[self.first + used:] == FILL).all())
        return self.whole[self.first:self.first + used]


def _sentinelled(size: int, lead: int) -> Sentinelled:
    import torch
    whole = torch.full((GUARD + lead + size + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 16 == 0
    return Sentinelled(whole, GUARD + lead, size)


class Workspace(NamedTuple):
    whole: object
    nbytes: int

    def ptr(self) -> int:
        return self.whole.data_ptr() + 1

    def untouched_around(self):
        assert int(self.whole[0]) == WS_FILL and bool((self.whole[1 + self.nbytes:] == WS_FILL).all())


def _workspace(nbytes: int) -> Workspace:
    """Exactly ``nbytes`` inside WS_FILL bytes, one byte behind a 256-byte boundary: the library's own alignment of the
    base then leaves a single byte of the room it asks for that, so that an array that runs over its layout by an entry
    runs into the sentinels."""
    import torch
    whole = torch.full((1 + nbytes + GUARD,), WS_FILL, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 256 == 0
    return Workspace(whole, nbytes)


def _offsets_out(n: int):
    import torch
    return torch.full((n + 1 + 8,), OFF_FILL, dtype=torch.int64, device="cuda")


def _gather_call(fn, check, ws_bytes: int, head, batches, n: int, extra, codes, totals):
    """One call of a library's entry point that ends in gf_pp_k_gather, as its binding makes it, but with the workspace
    and every output inside sentinels: [(bases, qualities, offsets)] per side, as the call left them."""
    import torch
    outs = [(_sentinelled(int(b.bases.numel()), LEADS[s]), _sentinelled(int(b.bases.numel()), (LEADS[s] + 5) % 16),
             _offsets_out(n)) for s, b in enumerate(batches)]
    ws = _workspace(ws_bytes)
    ins = [[b.bases.data_ptr(), b.quals.data_ptr(), b.offsets.data_ptr()] for b in batches] + [[None] * 3] * (2 - len(batches))
    to = [[ob.ptr(), oq.ptr(), off.data_ptr()] for ob, oq, off in outs] + [[None] * 3] * (2 - len(batches))
    check(fn(*head, *ins[0], *ins[1], n, *extra, ws.ptr(), ws_bytes, *to[0], *to[1], codes.data_ptr(), totals.data_ptr(),
             torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    ws.untouched_around()
    return outs


def _held_to_the_plan(pool: Pool, plan: Plan, outs, raw: bool, what):
    """Offsets, bases and qualities of every side against the plan."""
    for s, (ob, oq, off) in enumerate(outs):
        total = int(plan.out_off[s][-1])
        if raw:
            o = off.cpu().numpy()
            assert (o[plan.n + 1:] == OFF_FILL).all(), what
            _same_array(o[:plan.n + 1], plan.out_off[s], (what, s, "offsets"))
            ob, oq = ob.part(total), oq.part(total)
        else:
            _same_array(off, plan.out_off[s], (what, s, "offsets"))
            ob, oq = ob[:total], oq[:total]
        _same_bytes(ob, _joined([o[0] for o in pool.outs[s]], plan.seq, plan.live), (what, s, "bases"))
        _same_bytes(oq, _joined([o[1] for o in pool.outs[s]], plan.seq, plan.live), (what, s, "qualities"))


def _codes_of(pool: Pool, plan: Plan) -> np.ndarray:
    return np.concatenate([col[plan.seq] for col in pool.codes])


MODES = [pytest.param(1, id="single-end"), pytest.param(2, id="paired")]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("sides", MODES)
def test_read_filter(ix, sides, shape):
    import torch
    from genefuserust_amd import read_filter as rf
    pool, plan = library_plan("filter", sides, shape)
    n = plan.n
    batches = [_records_batch(pool.ins[s], plan, LEADS[s]) for s in range(sides)]
    config = rf.ReadFilter(*FILTER_SETTINGS)
    *got, totals, why = rf.filter_reads_device(ix, config, *batches, reasons=True)
    _held_to_the_plan(pool, plan, [(b.bases, b.quals, b.offsets) for b in got], False, "filter_reads_device")
    _same_array(why, _codes_of(pool, plan), "reasons")
    assert totals.cpu().tolist() == plan.totals.tolist()
    L = rf.lib()
    settings = rf.GfPpSettings(*FILTER_SETTINGS)
    why = torch.full((n * sides + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    totals = torch.full((8 + 8,), OFF_FILL, dtype=torch.int64, device="cuda")
    outs = _gather_call(L.gf_pp_filter_device, rf.check, int(L.gf_pp_workspace_bytes(n)), [ix._handle(), C.byref(settings)],
                        batches, n, [], why, totals)
    _held_to_the_plan(pool, plan, outs, True, "gf_pp_filter_device")
    _same_array(why[:n * sides], _codes_of(pool, plan), "reasons")
    assert bool((why[n * sides:] == FILL).all())
    assert totals.cpu().tolist() == plan.totals.tolist() + [OFF_FILL] * 8


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("sides", MODES)
def test_adapter_trimming(ix, sides, shape):
    import torch
    from genefuserust_amd import adapter_trim as at
    pool, plan = library_plan("adapter", sides, shape)
    n, s = plan.n, pool.more["settings"]
    batches = [_records_batch(pool.ins[k], plan, LEADS[k]) for k in range(sides)]
    config = at.AdapterTrim(bool(s.overlap), s.adapter_r1.decode(), s.adapter_r2.decode(), s.min_overlap, s.max_diff,
                            s.diff_percent, s.min_adapter)
    *got, totals, how = at.trim_adapters_device(ix, config, *batches, how=True)
    _held_to_the_plan(pool, plan, [(b.bases, b.quals, b.offsets) for b in got], False, "trim_adapters_device")
    _same_array(how, _codes_of(pool, plan), "how")
    assert totals.cpu().tolist() == plan.totals.tolist()
    L = at.lib()
    settings = at.settings_of(config)
    how = torch.full((n * sides + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    totals = torch.full((at.TOTALS + 8,), OFF_FILL, dtype=torch.int64, device="cuda")
    outs = _gather_call(L.gf_at_trim_device, at.check, int(L.gf_at_workspace_bytes(n)), [ix._handle(), C.byref(settings)],
                        batches, n, [], how, totals)
    _held_to_the_plan(pool, plan, outs, True, "gf_at_trim_device")
    _same_array(how[:n * sides], _codes_of(pool, plan), "how")
    assert bool((how[n * sides:] == FILL).all())
    assert totals.cpu().tolist() == plan.totals.tolist() + [OFF_FILL] * 8


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("sides,source", [pytest.param(1, "read1", id="single-end-read1"),
                                          pytest.param(2, "read1", id="paired-read1"),
                                          pytest.param(2, "read2", id="paired-read2"),
                                          pytest.param(2, "per_read", id="paired-per_read")])
def test_umi_cut(ix, sides, source, shape):
    import torch
    from genefuserust_amd import umi as um
    pool = umi_pool(sides, source)
    plan = plan_of(pool, SHAPES[shape], seed=sum(shape.encode()) + sides)
    n = plan.n
    batches = [_records_batch(pool.ins[k], plan, LEADS[k]) for k in range(sides)]
    config = um.Umi(source, UMI_LENGTH, UMI_SKIP)
    *got, codes, totals = um.cut_umis_device(ix, config, *batches)
    _held_to_the_plan(pool, plan, [(b.bases, b.quals, b.offsets) for b in got], False, "cut_umis_device")
    _same_array(codes, _codes_of(pool, plan), "codes")
    assert totals.cpu().tolist() == plan.totals.tolist() and plan.totals[5] > 0
    L = um.lib()
    settings = config.settings()
    codes = torch.full((n + GUARD,), OFF_FILL, dtype=torch.int64, device="cuda")
    before = [3, 0, 5, 0, 7, 0, 11]                     # (the cut adds into the totals)
    totals = torch.tensor(before + [OFF_FILL] * 8, dtype=torch.int64, device="cuda")
    outs = _gather_call(L.gf_um_cut_device, um.check, int(L.gf_um_workspace_bytes(n)), [ix._handle(), C.addressof(settings)],
                        batches, n, [], codes, totals)
    _held_to_the_plan(pool, plan, outs, True, "gf_um_cut_device")
    _same_array(codes[:n], _codes_of(pool, plan), "codes")
    assert bool((codes[n:] == OFF_FILL).all())
    assert totals.cpu().tolist() == [a + b for a, b in zip(plan.totals.tolist(), before)] + [OFF_FILL] * 8


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("sides", MODES)
def test_duplicate_removal(ix, sides, shape):
    """The duplicate pattern is laid into the table, not made by inserting: record i has slot i (none without bases), and
    the table says that the first record of its key is i itself, or the record in front of it for a duplicate — copies of
    256 entries inserted would leave only the first 256 records, and every tile sum past the first tiles 0."""
    import torch
    from genefuserust_amd import dedup as dd
    pool, plan = library_plan("dedup", sides, shape)
    n = plan.n
    assert n <= DEDUP_SLOTS
    batches = [_records_batch(pool.ins[k], plan, LEADS[k]) for k in range(sides)]
    has_bases = pool.had().sum(axis=0)[plan.seq] > 0
    at = np.arange(n, dtype=np.int64)
    first = np.full(DEDUP_SLOTS, dd.NO_INDEX, dtype=np.int64)
    first[:n] = np.where(has_bases, FIRST_INDEX + at - (1 - plan.live), dd.NO_INDEX)
    table = dd.Table(torch.zeros(DEDUP_SLOTS, dtype=torch.int64, device="cuda"), torch.from_numpy(first).cuda(), None)
    rec_slot = torch.from_numpy(np.where(has_bases, at, -1)).cuda()
    dup_want = (1 - plan.live).astype(np.uint8)
    removed = int((pool.had().sum(axis=0)[plan.seq] * (1 - plan.live)).sum())
    assert 0.4 < dup_want.mean() < 0.5 and (~has_bases).sum() > 0
    before = [3, 5, 7, 11, 13, 0]
    want_totals = [3, 5, 7, 11 + int(dup_want.sum()), 13 + removed, 0]
    totals = torch.tensor(before, dtype=torch.int64, device="cuda")
    *got, dup = dd.remove_device(ix, rec_slot, FIRST_INDEX, table, totals, *batches)
    _held_to_the_plan(pool, plan, [(b.bases, b.quals, b.offsets) for b in got], False, "remove_device")
    _same_array(dup, dup_want, "dup")
    assert totals.cpu().tolist() == want_totals
    L = dd.lib()
    dup = torch.full((n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    totals = torch.tensor(before + [OFF_FILL] * 8, dtype=torch.int64, device="cuda")
    outs = _gather_call(L.gf_dd_remove_device, dd.check, int(L.gf_dd_workspace_bytes(n)), [ix._handle()], batches, n,
                        [FIRST_INDEX, rec_slot.data_ptr(), table.first.data_ptr()], dup, totals)
    _held_to_the_plan(pool, plan, outs, True, "gf_dd_remove_device")
    _same_array(dup[:n], dup_want, "dup")
    assert bool((dup[n:] == FILL).all())
    assert totals.cpu().tolist() == want_totals + [OFF_FILL] * 8
    assert torch.equal(table.first.cpu(), torch.from_numpy(first))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("tagged", [pytest.param(False, id="plain"), pytest.param(True, id="tagged")])
@pytest.mark.parametrize("sides", MODES)
def test_writer(ix, sides, tagged, shape):
    """The FASTQ text of each side is cut on the device; the records the steps left are laid beside it at leads of their
    own.  format_reads_device, then the entry point with both gathers, the workspace and the out texts inside
    sentinels."""
    import torch
    from genefuserust_amd import read_write as rw
    from genefuserust_amd.fastq import fastq_cut_device
    from genefuserust_amd.umi import Umi
    pool = writer_pool(sides, tagged)
    plan = plan_of(pool, SHAPES[shape], seed=sum(shape.encode()) + sides)
    n = plan.n
    d_texts = [_up(_joined(side, plan.seq)) for side in pool.ins]
    cuts = [fastq_cut_device(ix, t) for t in d_texts]
    assert all(int(c.n_records) == n and int(c.n_bad_quality) == 0 for c in cuts)
    finals = [_records_batch(pool.more["finals"][s], plan, LEADS[s]) for s in range(sides)]
    want_texts = [_joined(side, plan.seq) for side in pool.outs]
    tag = dict(pre=cuts, umi=Umi("per_read", UMI_LENGTH, UMI_SKIP)) if tagged else {}
    out_texts, out_offs, totals = rw.format_reads_device(ix, d_texts, cuts, finals, n, **tag)
    assert totals.cpu().tolist() == plan.totals.tolist() and 0.25 * n < plan.totals[4] < 0.45 * n
    for s in range(sides):
        _same_array(out_offs[s], plan.out_off[s], ("format_reads_device", s, "offsets"))
        _same_bytes(out_texts[s][:len(want_texts[s])], want_texts[s], ("format_reads_device", s, "text"))
    L = rw.lib()
    ws_bytes = int(L.gf_rw_workspace_bytes(n))
    settings = rw.GfRwSettings(pool.more["source"], pool.more["length"], 0)
    for gather in (rw.WIDE, rw.BYTES):
        settings.gather = gather
        outs = [(_sentinelled(rw.capacity(int(t.numel()), n), (LEADS[s] + 4) % 16), _offsets_out(n))
                for s, t in enumerate(d_texts)]
        structs = [rw.GfRwSide(t.data_ptr(), int(t.numel()), c.nl_pos.data_ptr(), int(c.n_newlines), f.bases.data_ptr(),
                               f.quals.data_ptr(), f.offsets.data_ptr(), c.bases.data_ptr() if tagged else None,
                               c.offsets.data_ptr() if tagged else None, out.ptr(), out.size, off.data_ptr())
                   for t, c, f, (out, off) in zip(d_texts, cuts, finals, outs)]
        ws = _workspace(ws_bytes)
        before = [1000, 0, 5, 0, 7]
        totals = torch.tensor(before + [OFF_FILL] * 8, dtype=torch.int64, device="cuda")
        rw.check(L.gf_rw_format_device(ix._handle(), C.addressof(settings), C.addressof(structs[0]),
                                       C.addressof(structs[1]) if sides == 2 else None, n, ws.ptr(), ws_bytes,
                                       totals.data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        ws.untouched_around()
        assert totals.cpu().tolist() == [a + b for a, b in zip(plan.totals.tolist(), before)] + [OFF_FILL] * 8
        for s, (out, off) in enumerate(outs):
            o = off.cpu().numpy()
            assert (o[n + 1:] == OFF_FILL).all()
            _same_array(o[:n + 1], plan.out_off[s], ("gf_rw_format_device", gather, s, "offsets"))
            _same_bytes(out.part(len(want_texts[s])), want_texts[s], ("gf_rw_format_device", gather, s, "text"))
