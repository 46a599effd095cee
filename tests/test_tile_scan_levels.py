"""The tile scan of libgfmatch.so at every structural level: gf_scan_round, gf_k_compact_scan, gf_k_compact_scan_rounds and
gf_k_compact_scan_add (csrc/gf_compact_kernels.h), launch_scan and launch_scan_big (gfmatch.hip), through the three entry
points that take synthetic device inputs and need no mapping: gf_compact_hits_device (K4), gf_fastq_index_device and
gf_fastq_gather_device / gf_fastq_gather_lean_device.  One block of 1024 threads scans the per-tile totals, ROUND of them
per round: sixteen rows of ROW totals, each row scanned inside its wavefronts, the 16 x 16 wavefront sums through LDS.
The levels are the second wavefront of a row (past 64 totals), the second row (past ROW), the second round with its
``run`` carry and the reuse of the LDS sums (past ROUND), the switch to three launches (past 2 * ROUND, the newline index
only) and the ``base == 0`` early return of the third launch.  Every size below is a formula over the constants named
first — T whole tiles, and T tiles of which the last holds a single element, for every threshold T — and a test without
a GPU holds the constants to the sources' ``#define``s.

Nearly every tile is empty or sparse, so the expected output is a plain numpy statement over a few thousand planted
elements: the hit records from ``counts`` and ``matches`` alone, the newline positions as they were planted, the records
of a FASTQ text from the per-record arrays the text was built from.  Without a GPU the models are held to byte loops and
the text builder to ``oracle.fastq_cut``."""
import json
import os
import re
import struct
from typing import NamedTuple

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genefuserust_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "branch_cases.json")

WAVE = 64                       # lanes of a wavefront
CTHREADS = 256                  # GF_CTHREADS: the per-tile kernels' block
CTILE = 4096                    # GF_CTILE: count bytes per tile of K4
CPER = CTILE // CTHREADS        # GF_CPER: a thread's count bytes, one 16-byte load
FQ_TILE = 16384                 # GF_FQ_TILE: text bytes per tile of the newline index
FQ_PER = FQ_TILE // CTHREADS    # GF_FQ_PER: a thread's piece of the text
FQ_RTILE = 256                  # GF_FQ_RTILE: records per tile of the gather
ROW = 1024                      # the scan block: a row is one total per thread
SCAN_ROWS = 16                  # GF_SCAN_ROWS
ROUND = SCAN_ROWS * ROW         # GF_SCAN_ROUND
ONE_LAUNCH_ROUNDS = 2           # launch_scan_big: up to this many rounds stay with the one-block loop
THRESHOLDS = (1, WAVE, WAVE + 1, ROW, ROW + 1, ROUND, ROUND + 1, 2 * ROUND, 2 * ROUND + 1)
GATHER_THRESHOLDS = THRESHOLDS[:7]   # the gather's scan is launch_scan: one launch whatever the size
SIZES = [(T, kind) for T in THRESHOLDS for kind in ("whole", "single")]
GATHER_SIZES = [(T, kind) for T in GATHER_THRESHOLDS for kind in ("whole", "single")]
FILL = 0xEE
GUARD = 64                      # sentinel elements behind every capacity
NON_HITS = (3, 4, 127, 128, 254, 255)
DENSE_TILES = 70                # a run of fully hit tiles: 70 * 4096 > 2^18 in the wavefront bases
PLANT_LENS = (1, 15, 16, 17, 31, 150, 300)
RANDOM_TILES = 300


def size_of(T: int, kind: str, tile: int) -> int:
    """T whole tiles, or T tiles of which the last holds one element."""
    return T * tile if kind == "whole" else (T - 1) * tile + 1


def scan_route(ntiles: int):
    """(rounds, launches that launch_scan_big makes of them)."""
    rounds = -(-ntiles // ROUND)
    return rounds, 1 if rounds <= ONE_LAUNCH_ROUNDS else 3


def boundary_tiles(ntiles: int):
    """The tiles just below, at and just above every threshold (tile T - 1 is the last of its level, tile T the first
    of the next), the first tile and the last."""
    out = {0, ntiles - 1}
    for th in THRESHOLDS:
        out |= {t for t in (th - 2, th - 1, th) if 0 <= t < ntiles}
    return sorted(out)


# ---- 0. the sizes are the sources' ---------------------------------------------------------------------------------

def _define(header: str, name: str) -> str:
    src = open(os.path.join(CSRC, header)).read()
    m = re.search(r"^#define\s+%s\s+(.+?)\s*(?://.*)?$" % name, src, flags=re.M)
    assert m, (header, name)
    return m.group(1)


def test_sizes_are_the_sources_defines():
    assert int(_define("gf_compact_kernels.h", "GF_CTILE")) == CTILE
    assert int(_define("gf_compact_kernels.h", "GF_CTHREADS")) == CTHREADS
    assert _define("gf_compact_kernels.h", "GF_CPER") == "(GF_CTILE / GF_CTHREADS)"
    assert int(_define("gf_compact_kernels.h", "GF_SCAN_ROWS")) == SCAN_ROWS
    assert _define("gf_compact_kernels.h", "GF_SCAN_ROUND") == "(%d * GF_SCAN_ROWS)" % ROW
    assert int(_define("gf_fastq_kernels.h", "GF_FQ_TILE")) == FQ_TILE
    assert _define("gf_fastq_kernels.h", "GF_FQ_PER") == "(GF_FQ_TILE / GF_CTHREADS)"
    assert int(_define("gf_fastq_kernels.h", "GF_FQ_RTILE")) == FQ_RTILE
    src = open(os.path.join(CSRC, "gf_compact_kernels.h")).read()
    # the scan block is ROW threads, a row one total per thread, and a round is walked in steps of GF_SCAN_ROUND
    assert len(re.findall(r"__launch_bounds__\(%d\) void gf_k_compact_scan" % ROW, src)) == 3
    assert len(re.findall(r"\(int64_t\)k \* %d" % ROW, src)) == 4
    assert "b0 += GF_SCAN_ROUND" in src and "if (base == 0) return;" in src
    # launch_scan_big: one launch up to ONE_LAUNCH_ROUNDS rounds, three above; every scan kernel a block of ROW
    host = open(os.path.join(CSRC, "gfmatch.hip")).read()
    m = re.search(r"static void launch_scan_big\(.*?\n}\n", host, flags=re.S)
    assert m
    big = m.group(0)
    assert re.search(r"if \(nr <= (\d+)\) \{\s*launch_scan\(", big).group(1) == str(ONE_LAUNCH_ROUNDS)
    assert len(re.findall(r"dim3\(\(unsigned\)nr\), dim3\(%d\)" % ROW, big)) == 2
    assert "(ntiles + GF_SCAN_ROUND - 1) / GF_SCAN_ROUND" in host
    # which scan each entry point takes
    body = lambda name: re.search(r"\n(?:static )?int %s\(.*?\n}\n" % name, host, flags=re.S).group(0)
    assert "launch_scan(st, ntiles, tile_counts, tile_offsets, (int64_t*)d_n_hits)" in body("gf_compact_hits_device")
    assert "launch_scan_big(st, ntiles, tile_counts, tile_offsets, n_lines + 1" in body("gf_fastq_index_device")
    assert "launch_scan(st, ntiles, tile_counts, tile_offsets, total)" in body("fastq_gather_impl")


def test_sizes_cross_the_thresholds():
    for T, kind in SIZES:
        for tile in (CTILE, FQ_TILE, FQ_RTILE):
            n = size_of(T, kind, tile)
            assert -(-n // tile) == T and (n % tile == 0) == (kind == "whole" or tile == 1)
    route = {T: scan_route(T) for T in THRESHOLDS}
    assert [route[T] for T in THRESHOLDS] == [(1, 1)] * 6 + [(2, 1), (2, 1), (3, 3)]
    assert ROW // WAVE == 16 and ROUND == 16384   # (s_w: 16 rows of 16 wavefront sums)
    # the last total of a level and the first of the next are both boundary tiles at every size that has them
    for T in THRESHOLDS:
        b = boundary_tiles(T)
        assert 0 in b and T - 1 in b and all(th - 1 in b for th in THRESHOLDS if th <= T)
        assert all(th in b for th in THRESHOLDS if th < T)


# ---- 1. K4: gf_compact_hits_device against numpy --------------------------------------------------------------------

def compact_model(c: np.ndarray, base: int, take):
    """(indices of the hit reads, their gf_hit records) from the count bytes and ``take(idx)`` = matches[idx]."""
    from genefuserust_amd._lib import HIT_DTYPE
    idx = np.flatnonzero((c == 1) | (c == 2))
    rows = take(idx)
    rec = np.zeros(idx.size, dtype=HIT_DTYPE)
    rec["read_id"] = base + idx
    rec["n"] = c[idx]
    m = rec["m"]
    m[:, 0] = rows[:, 0]
    two = c[idx] == 2
    m[two, 1] = rows[two, 1]
    return idx, rec


def compact_byte_loop(c: np.ndarray, matches: np.ndarray, base: int) -> bytes:
    out = bytearray()
    for r in range(len(c)):
        if c[r] == 1 or c[r] == 2:
            out += struct.pack("<qii", base + r, int(c[r]), 0) + matches[r, 0].tobytes()
            out += matches[r, 1].tobytes() if c[r] == 2 else bytes(16)
    return bytes(out)


def dense_tiles(ntiles: int, first: int = 2):
    """The run of fully hit tiles: DENSE_TILES of them across the boundary of the first two wavefronts where the batch
    has room, fewer below that, none in a batch of a few tiles."""
    return range(first, min(first + DENSE_TILES, ntiles - 2)) if ntiles - 2 > first else range(0)


def compaction_counts(n: int, seed: int = 1, empty_first_round: bool = False) -> np.ndarray:
    """The count bytes of a batch of n reads: zero but for a run of fully hit tiles (counts 1 and 2 in turn) in front of
    sparse ones, hits at the first and last read of every boundary tile with non-hit bytes next to them, and a few
    thousand hits and non-hit bytes anywhere.  ``empty_first_round``: no hit among the first ROUND tiles."""
    rng = np.random.default_rng(seed)
    c = np.zeros(n, dtype=np.uint8)
    if n == 0:
        return c
    ntiles = -(-n // CTILE)
    where = rng.integers(0, n, size=min(n // 8, 6000))
    c[where] = np.resize(np.array(NON_HITS + (1, 2, 0), dtype=np.uint8), where.size)
    dense = dense_tiles(ntiles, ROUND + 2 if empty_first_round else 2)
    if len(dense):
        run = c[dense.start * CTILE:dense.stop * CTILE]
        run[:] = np.resize(np.array([1, 2, 2, 1, 1], dtype=np.uint8), run.size)
    turn = 0
    for t in boundary_tiles(ntiles):
        first, last = t * CTILE, min((t + 1) * CTILE, n) - 1
        for p, q in ((first, first + 1), (last, last - 1)):
            if first <= q <= last and c[q] not in (1, 2):
                c[q] = NON_HITS[turn % len(NON_HITS)]
            c[p] = 1 + turn % 2
            turn += 1
    if empty_first_round:
        head = c[:ROUND * CTILE]
        head[head == 1] = 3
        head[head == 2] = 254
    return c


def compaction_caps(c: np.ndarray):
    """0, one short, a value that ends inside a fully hit tile (in the middle of the list where there is none), ten
    more than there are."""
    hit = (c == 1) | (c == 2)
    total = int(hit.sum())
    tiles = hit[:c.size // CTILE * CTILE].reshape(-1, CTILE).sum(axis=1)
    full = np.flatnonzero(tiles == CTILE)
    inside = int(tiles[:full[min(3, full.size - 1)]].sum()) + 1234 if full.size else total // 2
    return total, sorted({0, max(total - 1, 0), inside, total + 10})


def test_compaction_model_equals_the_byte_loop():
    from genefuserust_amd._lib import SEQMATCH_DTYPE
    rng = np.random.default_rng(3)
    for n in (0, 1, 15, 16, 17, 500, 3000):
        c = rng.choice(np.array((0, 0, 0, 1, 2) + NON_HITS, dtype=np.uint8), size=n)
        matches = rng.integers(1, 32767, size=(n, 16), dtype=np.int16).view(SEQMATCH_DTYPE).reshape(n, 2)
        idx, rec = compact_model(c, 2 ** 40 + 7, lambda i: matches[i])
        assert rec.tobytes() == compact_byte_loop(c, matches, 2 ** 40 + 7)
        assert (rec["pad"] == 0).all() and idx.size == int(((c == 1) | (c == 2)).sum())
        if n >= 500:
            assert (rec["n"] == 1).any() and (rec["n"] == 2).any() and set(NON_HITS) <= set(c.tolist())


def test_compaction_counts_reach_every_level():
    for T, kind in SIZES[:10]:   # (the sizes of a whole round and more are built on the GPU machine only: 67 to 134 MB)
        n = size_of(T, kind, CTILE)
        c = compaction_counts(n, seed=T)
        ntiles = -(-n // CTILE)
        total, caps = compaction_caps(c)
        hit = (c == 1) | (c == 2)
        assert hit[0] and hit[n - 1] and total >= 1
        for t in boundary_tiles(ntiles):
            assert hit[t * CTILE] and hit[min((t + 1) * CTILE, n) - 1]
        if n > 16 * CTILE:
            assert set(NON_HITS) <= set(np.unique(c).tolist()) and {1, 2} <= set(c[hit].tolist())
        d = dense_tiles(ntiles)
        assert len(d) == (DENSE_TILES if T >= ROW else max(0, min(DENSE_TILES, ntiles - 4)))
        if len(d):
            assert hit[d.start * CTILE:d.stop * CTILE].all()
            before = int(hit[:d.start * CTILE].sum())
            inside = [x for x in caps if before < x < before + len(d) * CTILE and (x - before) % CTILE]
            assert inside, (T, kind, caps)
        if T >= ROW:   # sums past 2^18 in front of sparse tiles, in every wavefront's base behind the run
            assert len(d) * CTILE > 2 ** 18 and d.start < WAVE < d.stop and ntiles - d.stop > 900
            sums = hit[:n // CTILE * CTILE].reshape(-1, CTILE).sum(axis=1)
            assert (sums[d.stop:] > 0).sum() >= 200 and (sums[d.stop:] == 0).sum() >= 100


def _cuda_index(gpu_device):
    from genefuserust_amd import Indexer
    g = json.load(open(GOLDEN))
    ix = Indexer.from_gene_slices([None if x is None else x.encode() for x in g["genes"]], g["reversed"])
    ix.make_index()
    return ix


@pytest.fixture(scope="module")
def small_index(gpu_device):
    ix = _cuda_index(gpu_device)
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def garbage_matches(gpu_device):
    """matches[n][2] for the largest batch, every 16-bit half of every field non-zero, ``pad`` included: allocated once
    (4.3 GB), every case takes a prefix of it, freed with the module."""
    import torch
    rows = THRESHOLDS[-1] * CTILE
    g = torch.empty((rows, 16), dtype=torch.int16, device="cuda")
    step = 1 << 22
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4)
    for lo in range(0, rows, step):
        g[lo:lo + step].random_(1, 32767, generator=gen)
    yield g
    del g
    torch.cuda.empty_cache()


def _first_bad(got: np.ndarray, want: np.ndarray) -> int:
    bad = np.flatnonzero(got != want)
    return int(bad[0]) if bad.size else -1


def _run_compaction(ix, garbage, c, base, counts_shift=None):
    """gf_compact_hits_device over the count bytes ``c`` and a prefix of the garbage matches, at every capacity of
    compaction_caps: the true total, exactly the first min(cap, total) records, the sentinels behind them."""
    import torch
    from genefuserust_amd import _lib
    from genefuserust_amd._lib import SEQMATCH_DTYPE
    L, h = _lib.lib(), ix._handle()
    n = c.size
    st = torch.cuda.current_stream().cuda_stream
    if counts_shift is None:
        d_counts = torch.from_numpy(c).cuda()
    else:
        raw = torch.zeros(n + 32, dtype=torch.uint8, device="cuda")
        assert raw.data_ptr() % 16 == 0
        d_counts = raw[counts_shift:counts_shift + n]
        d_counts.copy_(torch.from_numpy(c))
    take = lambda i: garbage[torch.from_numpy(i).cuda()].cpu().numpy().view(SEQMATCH_DTYPE).reshape(-1, 2)
    idx, want = compact_model(c, base, take)
    if idx.size:
        assert (want["m"]["pad"][:, 0] != 0).all() and (want["m"]["seq_end"][want["n"] == 2, 1] != 0).all()
    want = want.view(np.uint8).reshape(-1, 48)
    total, caps = compaction_caps(c)
    assert total == idx.size
    ws = torch.empty(int(L.gf_compact_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    for cap in caps:
        hits = torch.full((cap + GUARD, 48), FILL, dtype=torch.uint8, device="cuda")
        n_hits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        _lib.check(L.gf_compact_hits_device(h, d_counts.data_ptr(), garbage.data_ptr(), n, base, hits.data_ptr(), cap,
                                            n_hits.data_ptr(), ws.data_ptr(), st))
        torch.cuda.synchronize()
        got = hits.cpu().numpy()
        w = min(cap, total)
        assert int(n_hits.item()) == total, (cap, int(n_hits.item()), total)
        bad = _first_bad(got[:w], want[:w])
        assert bad < 0, (cap, bad // 48, got[bad // 48].tobytes(), want[bad // 48].tobytes())
        assert (got[w:] == FILL).all(), (cap, w + _first_bad(got[w:], np.full_like(got[w:], FILL)) // 48)
    return total


@pytest.mark.gpu
@pytest.mark.parametrize("T,kind", SIZES)
def test_compaction_at_every_level(small_index, garbage_matches, T, kind):
    n = size_of(T, kind, CTILE)
    total = _run_compaction(small_index, garbage_matches, compaction_counts(n, seed=T), base=1000)
    assert total >= (DENSE_TILES * CTILE if T >= ROW else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ragged", "empty", "base 2^40", "first round empty", "counts + 1", "counts + 8"])
def test_compaction_edges(small_index, garbage_matches, case):
    if case == "ragged":          # n no multiple of 16: the last thread that has reads takes them byte by byte
        n = WAVE * CTILE + 5 * CPER + 11
        assert n % CPER and _run_compaction(small_index, garbage_matches, compaction_counts(n), base=0) > 0
    elif case == "empty":
        assert _run_compaction(small_index, garbage_matches, compaction_counts(0), base=5) == 0
    elif case == "base 2^40":
        n = size_of(ROW + 1, "single", CTILE)
        assert _run_compaction(small_index, garbage_matches, compaction_counts(n, seed=9), base=2 ** 40 + 7) > 0
    elif case == "first round empty":   # round 1 starts from run == 0, with the run of fully hit tiles in it
        n = size_of(2 * ROUND, "whole", CTILE)
        c = compaction_counts(n, seed=10, empty_first_round=True)
        assert not ((c[:ROUND * CTILE] == 1) | (c[:ROUND * CTILE] == 2)).any()
        assert _run_compaction(small_index, garbage_matches, c, base=1000) >= DENSE_TILES * CTILE
    else:                               # a pointer off the 16-byte grid: every thread takes the byte path
        shift = int(case.split("+")[1])
        n = size_of(WAVE + 1, "single" if shift == 1 else "whole", CTILE)
        assert _run_compaction(small_index, garbage_matches, compaction_counts(n, seed=shift), 1000, counts_shift=shift) > 0


# ---- 2. gf_fastq_index_device against the planted positions ---------------------------------------------------------

def newline_positions(n: int, seed: int = 1, empty_rounds: int = 0, dense: bool = True) -> np.ndarray:
    """Sorted positions of the newlines of a text of n bytes: the first and the last byte of every boundary tile, one
    tile of nothing but newlines ahead of the sparse ones, a few thousand anywhere; none in the first ``empty_rounds``
    rounds of tiles.  (The last byte is among them: the caller takes it out for a text that ends without one.)"""
    rng = np.random.default_rng(seed)
    ntiles = -(-n // FQ_TILE)
    pos = [rng.integers(0, n, size=min(n // 4, 4000))]
    for t in boundary_tiles(ntiles):
        pos.append(np.array([t * FQ_TILE, min((t + 1) * FQ_TILE, n) - 1]))
    if dense and ntiles > 3:
        pos.append(np.arange(FQ_TILE, 2 * FQ_TILE))
    pos = np.unique(np.concatenate(pos)).astype(np.int64)
    return pos[pos >= empty_rounds * ROUND * FQ_TILE]


def newline_byte_loop(text: bytes):
    pos = [i for i in range(len(text)) if text[i] == 10]
    return pos, [len(pos) + (1 if text and text[-1] != 10 else 0), len(pos)]


def test_newline_plan_equals_the_byte_loop_and_stays_in_capacity():
    for n in (1, 2, 63, 64, 65, 3 * FQ_TILE + 5, 5 * FQ_TILE):
        pos = newline_positions(n, seed=n)
        for end in (True, False):
            p = pos if end else pos[pos != n - 1]
            text = np.full(n, 0x41, dtype=np.uint8)
            text[p] = 10
            got, lines = newline_byte_loop(text.tobytes())
            assert got == p.tolist() and lines == [p.size + (0 if end else 1), p.size]
    for T, kind in SIZES:
        n = size_of(T, kind, FQ_TILE)
        pos = newline_positions(n, seed=T)
        per_tile = np.bincount(pos // FQ_TILE, minlength=T)
        assert per_tile.max() <= FQ_TILE and (T <= 3 or per_tile[1] == FQ_TILE)   # (what the scan's uint32 sums rest on)
        assert np.bincount(pos // (FQ_TILE * ROUND)).max() < 2 ** 32
        assert pos[0] == 0 and pos[-1] == n - 1 and pos.size <= FQ_TILE + 4100
        for t in boundary_tiles(T):
            assert t * FQ_TILE in pos and min((t + 1) * FQ_TILE, n) - 1 in pos
        if T > 3:   # half the count ends inside the tile of nothing but newlines
            assert per_tile[0] < pos.size // 2 < per_tile[0] + FQ_TILE
    late = newline_positions(size_of(2 * ROUND + 1, "whole", FQ_TILE), empty_rounds=2)
    assert late.size >= 2 and late[0] == 2 * ROUND * FQ_TILE


def _text_on_device(n: int, pos: np.ndarray, shift: int = 0):
    import torch
    raw = torch.full((n + 16,), 0x41, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 16 == 0
    text = raw[shift:shift + n]
    if pos.size:
        text[torch.from_numpy(pos).cuda()] = 10
    return text


def _run_index(ix, text, n: int, want: np.ndarray, cap: int, ends_with_newline: bool):
    import torch
    from genefuserust_amd import _lib
    L = _lib.lib()
    ws = torch.empty(int(L.gf_fastq_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    nl = torch.full((cap + GUARD,), -7, dtype=torch.int64, device="cuda")
    n_lines = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    _lib.check(L.gf_fastq_index_device(ix._handle(), text.data_ptr(), n, nl.data_ptr(), cap, n_lines.data_ptr(),
                                       ws.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert n_lines.cpu().tolist() == [want.size + (0 if ends_with_newline or n == 0 else 1), want.size]
    got = nl.cpu().numpy()
    w = min(cap, want.size)
    bad = _first_bad(got[:w], want[:w])
    assert bad < 0, (cap, bad, int(got[bad]), int(want[bad]))
    assert (got[w:] == -7).all(), cap
    return nl


def _index_case(ix, n: int, pos: np.ndarray, shift: int = 0):
    """The text with a newline as its last byte, at a capacity with room and at half the count; then the same text with
    another last byte."""
    text = _text_on_device(n, pos, shift)
    assert pos[-1] == n - 1
    _run_index(ix, text, n, pos, pos.size + 10, True)
    _run_index(ix, text, n, pos, pos.size // 2, True)
    text[n - 1] = 0x41
    _run_index(ix, text, n, pos[:-1], pos.size + 10, False)


@pytest.mark.gpu
@pytest.mark.parametrize("T,kind", SIZES)
def test_newline_index_at_every_level(small_index, T, kind):
    n = size_of(T, kind, FQ_TILE)
    _index_case(small_index, n, newline_positions(n, seed=T))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ragged", "empty", "only round 2", "round 1 empty", "text + 1", "text + 5"])
def test_newline_index_edges(small_index, case):
    if case == "ragged":        # n_bytes no multiple of 64: the last thread that has text takes it byte by byte
        n = WAVE * FQ_TILE + 3 * FQ_PER + 37
        assert n % FQ_PER
        _index_case(small_index, n, newline_positions(n, seed=2))
    elif case == "empty":
        _run_index(small_index, _text_on_device(0, np.zeros(0, np.int64)), 0, np.zeros(0, np.int64), 4, False)
    elif case == "only round 2":    # three launches, and every round's base is 0
        n = size_of(2 * ROUND + 1, "whole", FQ_TILE)
        _index_case(small_index, n, newline_positions(n, seed=3, empty_rounds=2))
    elif case == "round 1 empty":   # rounds 1 and 2 have the same base, round 1 adds it to nothing
        n = size_of(2 * ROUND + 1, "whole", FQ_TILE)
        pos = newline_positions(n, seed=4)
        pos = pos[(pos < ROUND * FQ_TILE) | (pos >= 2 * ROUND * FQ_TILE)]
        _index_case(small_index, n, pos)
    else:                           # a text off the 16-byte grid: every thread takes the byte path
        shift = int(case.split("+")[1])
        n = size_of(WAVE + 1, "single" if shift == 1 else "whole", FQ_TILE)
        _index_case(small_index, n, newline_positions(n, seed=shift), shift=shift)


def every_byte_text() -> np.ndarray:
    """Four tiles in which thread t's byte p is (t + s * p) mod 256 for s = 0, 1, 3, 255 — every byte value at each of
    the 64 positions of a piece, with equal, rising and falling neighbours — and the values next to 0x0A in either
    nibble or the top bit, each between two newlines and between two others."""
    t, p = np.arange(CTHREADS)[:, None], np.arange(FQ_PER)[None, :]
    tiles = [((t + s * p) % 256).astype(np.uint8).reshape(-1) for s in (0, 1, 3, 255)]
    near = bytes([0x8A, 0x0B, 0x1A, 0x00, 0xFF, 0x09, 0x2A, 0x4A, 0x0E, 0x02, 0x08, 0x7A, 0x80, 0x7F, 0x0A])
    tail = b"".join(bytes([10, v, 10, 10, v, v, 10, v, 0x41, v, 0x41, 10]) for v in near)
    return np.concatenate(tiles + [np.frombuffer(tail, dtype=np.uint8)])


def test_every_byte_text_holds_every_value_at_every_place():
    text = every_byte_text()
    for k in range(4):
        tile = text[k * FQ_TILE:(k + 1) * FQ_TILE].reshape(CTHREADS, FQ_PER)
        assert all(len(set(tile[:, p].tolist())) == 256 for p in range(FQ_PER))
    pos, lines = newline_byte_loop(text.tobytes())
    assert pos == np.flatnonzero(text == 10).tolist() and len(pos) >= 4 * FQ_PER + 4 * 14


@pytest.mark.gpu
def test_newline_index_reports_0x0a_only(small_index):
    import torch
    text = every_byte_text()
    want = np.flatnonzero(text == 10).astype(np.int64)
    _run_index(small_index, torch.from_numpy(text).cuda(), text.size, want, want.size + 10, text[-1] == 10)


# ---- 3. gf_fastq_gather_device and gf_fastq_gather_lean_device against the builder -----------------------------------

class Fastq(NamedTuple):
    text: np.ndarray       # uint8
    nl_pos: np.ndarray     # int64: every newline of the text
    n_rec: int
    offsets: np.ndarray    # int64[n_rec + 1]
    bases: np.ndarray      # the sequence lines back to back
    quals: np.ndarray      # the quality lines cut or padded with '!' to their sequences' lengths
    qual_off: np.ndarray   # int64[n_rec]: where each quality line starts in the text
    n_bad: int
    names: tuple           # (start, length) of every name line, for the check against the oracle


def _ragged(at, lens, ids, a, b, c, mod, lo):
    """Byte k of element i (``lens[i]`` bytes at ``at[i]``) is lo + (ids[i] * a + k * b + k // c) % mod: (where, what)."""
    first = np.cumsum(lens) - lens
    k = np.arange(int(lens.sum())) - np.repeat(first, lens)
    r = np.repeat(ids, lens)
    return np.repeat(at, lens) + k, (lo + (r * a + k * b + k // c) % mod).astype(np.uint8)


def build_fastq(n_rec: int, rec, lens, short_quality=(), final_newline: bool = True) -> Fastq:
    """The text of n_rec records, and what its cut has to be, from per-record arrays: every record is the filler
    ``@ \\n \\n + \\n \\n`` (an empty sequence) but for records ``rec`` (ascending), which have a name of 1 .. 23 bytes and a
    sequence and a quality line of ``lens`` bytes that depend on the record's number and the byte's place; the quality
    lines of ``short_quality`` are one byte short."""
    rec, lens = np.asarray(rec, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    seq_len = np.zeros(n_rec, dtype=np.int64)
    seq_len[rec] = lens
    qual_len = seq_len.copy()
    qual_len[np.asarray(list(short_quality), dtype=np.int64)] -= 1
    name_len = np.ones(n_rec, dtype=np.int64)
    name_len[rec] = 1 + rec % 23
    size = name_len + seq_len + qual_len + 5                      # four newlines and the '+'
    s = np.cumsum(size) - size
    seq_at, plus_at = s + name_len + 1, s + name_len + seq_len + 2
    qual_at = plus_at + 2
    nl_pos = np.stack([s + name_len, seq_at + seq_len, plus_at + 1, qual_at + qual_len], axis=1).reshape(-1)
    text = np.zeros(int(size.sum()), dtype=np.uint8)
    text[nl_pos] = 10
    text[s] = ord("@")
    text[plus_at] = ord("+")
    at, what = _ragged(s[rec] + 1, name_len[rec] - 1, rec, 1, 1, 99, 26, ord("a"))
    text[at] = what
    at, bases = _ragged(seq_at[rec], seq_len[rec], rec, 13, 5, 16, 26, ord("A"))
    text[at] = bases
    at, q = _ragged(qual_at[rec], qual_len[rec], rec, 17, 3, 7, 60, 33)
    text[at] = q
    assert (text != 0).all()
    offsets = np.concatenate([[0], np.cumsum(seq_len)]).astype(np.int64)
    quals = np.full(int(offsets[-1]), ord("!"), dtype=np.uint8)
    quals[_ragged(offsets[rec], qual_len[rec], rec, 0, 0, 1, 1, 0)[0]] = q
    if not final_newline:
        text, nl_pos = text[:-1], nl_pos[:-1]
    return Fastq(text, nl_pos, n_rec, offsets, bases, quals, qual_at, len(list(short_quality)), (s, name_len))


def gather_plan(n_rec: int, seed: int = 1):
    """Which records are not fillers, and their lengths: in every boundary tile a run of consecutive records of every
    length at its first and at its last slots (pieces spliced from two records; the tile's edges mid-piece), short
    records with empty ones between them and a run of one-byte records (pieces over three and more records), records of
    150 and 300 bytes (whole pieces); a run of DENSE_TILES tiles without a filler in front of the sparse tiles; and one
    record in RANDOM_TILES further tiles."""
    ntiles = -(-n_rec // FQ_RTILE)
    rng = np.random.default_rng(seed)
    at = {}

    def put(r, ln):
        if 0 <= r < n_rec:
            at.setdefault(int(r), ln)

    for j, t in enumerate(boundary_tiles(ntiles)):
        r0 = t * FQ_RTILE
        room = min(FQ_RTILE, n_rec - r0)
        for i in range(len(PLANT_LENS)):
            put(r0 + i, PLANT_LENS[(i + j) % 7])
            if room - 7 + i >= 0:
                put(r0 + room - 7 + i, PLANT_LENS[(i + 2 * j + 3) % 7])
        if room == FQ_RTILE:
            for slot, ln in ((100, 1), (102, 15), (105, 1), (109, 17), (114, 1), (115, 31),          # empty ones between
                             (120, 1), (121, 1), (122, 1), (123, 1), (124, 1), (125, 1), (126, 150),  # ones in a row
                             (140, 150), (141, 300), (160, 300), (170, 16), (171, 16), (172, 16)):
                put(r0 + slot, ln)
    for t in dense_tiles(ntiles):
        for slot in range(FQ_RTILE):
            put(t * FQ_RTILE + slot, PLANT_LENS[(3 * slot + t) % 7])
    for t in rng.choice(ntiles, size=min(ntiles, RANDOM_TILES), replace=False):
        put(int(t) * FQ_RTILE + int(rng.integers(0, FQ_RTILE)), PLANT_LENS[int(rng.integers(0, 7))])
    rec = np.array(sorted(at), dtype=np.int64)
    return rec, np.array([at[int(r)] for r in rec], dtype=np.int64)


def piece_kinds(fq: Fastq) -> dict:
    """How many 16-byte pieces of the output each copy path of gf_k_fq_gather takes on an aligned output with room:
    'whole' (inside one record), 'splice' (the end of a record and the start of the next one of the tile), 'loop' (over
    three or more of the tile's records), 'skipped empty' (such a loop that steps over empty records) and 'edge' (a piece
    that a tile shares with its neighbour or that ends the output)."""
    kinds = {"whole": 0, "splice": 0, "loop": 0, "skipped empty": 0, "edge": 0}
    off = fq.offsets
    for t0 in range(0, fq.n_rec, FQ_RTILE):
        t1 = min(t0 + FQ_RTILE, fq.n_rec)
        pos0, end = int(off[t0]), int(off[t1])
        rel = off[t0:t1 + 1] - pos0
        for b0 in range(pos0 >> 4 << 4, end, 16):
            lo, hi = max(b0, pos0), min(b0 + 16, end)
            if lo >= hi:
                continue
            if lo != b0 or hi != b0 + 16:
                kinds["edge"] += 1
                continue
            i = int(np.searchsorted(rel, lo - pos0, side="right")) - 1       # the last record that starts at or before
            j = int(np.searchsorted(rel, hi - 1 - pos0, side="right")) - 1   # .. the piece's first and last byte
            nonempty = int((np.diff(rel[i:j + 2]) > 0).sum())
            if i == j:
                kinds["whole"] += 1
            elif j == i + 1:
                kinds["splice"] += 1
            else:
                kinds["loop"] += 1
                kinds["skipped empty"] += nonempty < j - i + 1
    return kinds


def _fastq_from_oracle(oracle, fq: Fastq):
    recs = oracle.fastq_cut(fq.text.tobytes())
    text = fq.text.tobytes()
    assert len(recs) == fq.n_rec
    s, name_len = fq.names
    assert [r[0] for r in recs] == [text[a:a + b] for a, b in zip(s.tolist(), name_len.tolist())]
    assert all(r[2] == b"+" for r in recs)
    assert fq.offsets.tolist() == np.concatenate([[0], np.cumsum([len(r[1]) for r in recs])]).tolist()
    assert fq.bases.tobytes() == b"".join(r[1] for r in recs)
    # a quality line is cut or padded with '!' to its sequence's length (include/gfmatch.h)
    assert fq.quals.tobytes() == b"".join(r[3][:len(r[1])] + b"!" * (len(r[1]) - len(r[3])) for r in recs)
    assert fq.n_bad == sum(len(r[1]) != len(r[3]) for r in recs)
    assert all(text[q:q + len(r[3])] == r[3] and (q == 0 or text[q - 1] == 10) for q, r in zip(fq.qual_off.tolist(), recs))
    assert fq.nl_pos.tolist() == np.flatnonzero(fq.text == 10).tolist()


def test_builder_equals_the_oracle_cut(oracle):
    for n_rec in (1, 2, FQ_RTILE - 1, FQ_RTILE + 1, size_of(WAVE + 1, "single", FQ_RTILE), 20_000):
        fq = build_fastq(n_rec, *gather_plan(n_rec, seed=n_rec))
        _fastq_from_oracle(oracle, fq)
    n_rec = size_of(WAVE + 1, "whole", FQ_RTILE)
    rec, lens = gather_plan(n_rec)
    short = WAVE * FQ_RTILE + 141
    assert short in rec and lens[rec == short] == 300
    _fastq_from_oracle(oracle, build_fastq(n_rec, rec, lens, short_quality=[short]))
    assert rec[-1] == n_rec - 1
    _fastq_from_oracle(oracle, build_fastq(n_rec, rec, lens, final_newline=False))


def test_gather_plan_reaches_every_path_and_level():
    for T, kind in GATHER_SIZES[:10]:   # (ROUND tiles and more are built on the GPU machine only)
        n_rec = size_of(T, kind, FQ_RTILE)
        rec, lens = gather_plan(n_rec, seed=T)
        fq = build_fastq(n_rec, rec, lens)
        assert rec[0] == 0 and rec[-1] == n_rec - 1 and set(lens.tolist()) <= set(PLANT_LENS)
        assert fq.text.size == 6 * n_rec + int((rec % 23).sum()) + 2 * int(lens.sum())
        sums = np.add.reduceat(np.diff(fq.offsets), np.arange(0, n_rec, FQ_RTILE))
        assert sums.size == T and sums[0] > 0 and sums[-1] > 0 and sums.max() < 2 ** 31
        if T >= WAVE:
            assert set(lens.tolist()) == set(PLANT_LENS)
        if T in (WAVE, WAVE + 1):
            kinds = piece_kinds(fq)
            assert all(kinds[k] >= least for k, least in (("whole", 100), ("splice", 100), ("loop", 8),
                                                          ("skipped empty", 4), ("edge", 20))), kinds
        if T >= WAVE:
            assert (fq.offsets[np.arange(0, n_rec, FQ_RTILE)] % 16 != 0).sum() >= 20     # tiles that begin mid-piece
        if T >= ROW:
            d = dense_tiles(T)
            assert len(d) == DENSE_TILES and sums[d.start:d.stop].sum() > 2 ** 18
            assert (sums[d.stop:] > 0).sum() >= 200 and (sums[d.stop:] == 0).sum() >= 100
    assert (ROUND + 1) * FQ_RTILE * 6 < 26_000_000   # the largest text: fillers of six bytes


def _run_gather(ix, fq: Fastq, d_text, d_nl, lean: bool, out_shift: int = 0):
    """One gather over the device text and newline positions given: every offset, every base and quality byte (or every
    quality offset), the count of odd quality lines, and the sentinels around the capacity handed over."""
    import torch
    from genefuserust_amd import _lib
    L, h = _lib.lib(), ix._handle()
    st = torch.cuda.current_stream().cuda_stream
    n, total = fq.text.size, int(fq.offsets[-1])
    ws = torch.empty(int(L.gf_fastq_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    offsets = torch.full((fq.n_rec + 1 + GUARD,), -7, dtype=torch.int64, device="cuda")
    raw = [torch.full((total + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    assert all(r.data_ptr() % 16 == 0 for r in raw)
    bases, quals = raw[0][out_shift:], raw[1][out_shift:]
    qual_off = torch.full((fq.n_rec + GUARD,), -7, dtype=torch.int64, device="cuda")
    n_bad = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    if lean:
        _lib.check(L.gf_fastq_gather_lean_device(h, d_text.data_ptr(), n, d_nl.data_ptr(), fq.nl_pos.size, fq.n_rec,
                                                 offsets.data_ptr(), bases.data_ptr(), total, qual_off.data_ptr(),
                                                 n_bad.data_ptr(), ws.data_ptr(), st))
    else:
        _lib.check(L.gf_fastq_gather_device(h, d_text.data_ptr(), n, d_nl.data_ptr(), fq.nl_pos.size, fq.n_rec,
                                            offsets.data_ptr(), bases.data_ptr(), quals.data_ptr(), total,
                                            n_bad.data_ptr(), ws.data_ptr(), st))
    torch.cuda.synchronize()
    what = ("lean" if lean else "full", out_shift)
    assert int(n_bad.item()) == fq.n_bad, what
    got = offsets.cpu().numpy()
    bad = _first_bad(got[:fq.n_rec + 1], fq.offsets)
    assert bad < 0, (what, "offsets", bad, int(got[bad]), int(fq.offsets[bad]))
    assert (got[fq.n_rec + 1:] == -7).all(), what
    outputs = [("bases", raw[0], fq.bases)]
    if lean:
        got = qual_off.cpu().numpy()
        bad = _first_bad(got[:fq.n_rec], fq.qual_off)
        assert bad < 0, (what, "qual_off", bad, int(got[bad]), int(fq.qual_off[bad]))
        assert (got[fq.n_rec:] == -7).all() and (raw[1] == FILL).all().item(), what
    else:
        outputs.append(("quals", raw[1], fq.quals))
    for name, r, want in outputs:
        got = r.cpu().numpy()
        assert (got[:out_shift] == FILL).all() and (got[out_shift + total:] == FILL).all(), (what, name)
        bad = _first_bad(got[out_shift:out_shift + total], want)
        rec = int(np.searchsorted(fq.offsets, bad, side="right")) - 1
        assert bad < 0, (what, name, bad, "record", rec, "tile", rec // FQ_RTILE, int(got[out_shift + bad]), int(want[bad]))


def _gather_case(ix, fq: Fastq, shifts=(0,), chain: bool = True):
    import torch
    d_text = torch.from_numpy(fq.text).cuda()
    d_nl = torch.from_numpy(fq.nl_pos).cuda()
    for shift in shifts:
        _run_gather(ix, fq, d_text, d_nl, lean=False, out_shift=shift)
        _run_gather(ix, fq, d_text, d_nl, lean=True, out_shift=shift)
    if chain:   # once per size the newline positions of gf_fastq_index_device instead of the builder's
        nl = _run_index(ix, d_text, fq.text.size, fq.nl_pos, fq.nl_pos.size + 10, fq.text[-1] == 10)
        _run_gather(ix, fq, d_text, nl, lean=False)


@pytest.mark.gpu
@pytest.mark.parametrize("T,kind", GATHER_SIZES + [(ROUND + 1, "and one")])
def test_gather_at_every_level(small_index, T, kind):
    """("and one": ROUND + 1 whole tiles and one record, the largest text: 25 MB.)"""
    n_rec = T * FQ_RTILE + 1 if kind == "and one" else size_of(T, kind, FQ_RTILE)
    _gather_case(small_index, build_fastq(n_rec, *gather_plan(n_rec, seed=T)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["short quality", "outputs + 1 and + 8", "no final newline"])
def test_gather_edges_at_the_second_wavefront(small_index, case):
    n_rec = size_of(WAVE + 1, "whole", FQ_RTILE)
    rec, lens = gather_plan(n_rec)
    if case == "short quality":     # in the first tile of the second wavefront: that tile alone a wavefront per record
        short = WAVE * FQ_RTILE + 141
        fq = build_fastq(n_rec, rec, lens, short_quality=[short])
        assert fq.n_bad == 1 and fq.quals[fq.offsets[short + 1] - 1] == ord("!")
        _gather_case(small_index, fq, chain=False)
    elif case == "outputs + 1 and + 8":   # off the 16-byte grid: every tile a wavefront per record
        _gather_case(small_index, build_fastq(n_rec, rec, lens), shifts=(1, 8), chain=False)
    else:
        fq = build_fastq(n_rec, rec, lens, final_newline=False)
        assert rec[-1] == n_rec - 1 and fq.text[-1] != 10 and fq.nl_pos.size == 4 * n_rec - 1
        _gather_case(small_index, fq)
