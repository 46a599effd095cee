"""The second level of the companion libraries' two-level scans: gf_se_k_scan (libgfse.so), gf_mc_k_scan (libgfmcsv.so),
gf_hn_k_scan (libgfnames.so), gf_rc_k_scan and gf_rc_k_name_scan (libgfrefcut.so).  The five kernels share one body
(gf_scan_totals_block, gf_scan_common.h) and keep their own tails.  One block of SCAN_THREADS threads scans the per-tile
totals; thread t takes a run of ``per = ceil(n / SCAN_THREADS)`` consecutive totals.  The other
modules stay at ``per = 1`` and inside one or two wavefronts of that block; here every batch is the smallest that
crosses a threshold — the second wavefront, runs of two and more totals, a shorter last run, trailing threads without a
run, a second iteration of the names' grid-stride loops — and nearly every element is a filler that gives nothing, so
the expected output is known by construction from a few dozen planted elements whose outcome the oracle chain gives.

Every size below is a formula over the constants named first, and a test without a GPU holds those constants to the
``#define``s of the sources: a later change of a tile size fails here and does not quietly bring the coverage back to
``per = 1``.  The same test holds the split into runs to one place, the shared body, and each kernel to its header."""
import os
import re
from typing import NamedTuple, Tuple

import numpy as np
import pytest

from tests.helpers import rand_seq, rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN_CSRC = os.path.join(ROOT, "genefuserust_amd", "scan_csrc")

WAVE = 64                           # lanes of a wavefront
BLOCK = 256                         # GF_SCAN_THREADS: the per-tile kernels' block
SCAN_THREADS = 1024                 # GF_SCAN_TOTALS_THREADS: the one block that scans the totals
SE_PER = 16                         # GF_SE_PER: reads per thread of a single-end tile
SE_TILE = BLOCK * SE_PER            # GF_SE_TILE
MC_TILE = BLOCK                     # GF_MC_TILE: one pair per thread
RC_PIECE = 16                       # GF_RC_PIECE; the tile itself is asked of the library (rc_tile())
HN_GRID_BLOCKS = 1024               # the cap of gf_hn_k_lengths' grid (gf_hit_names.hip)
HN_GRID_RECORDS = HN_GRID_BLOCKS * BLOCK   # records one iteration of its stride loop covers

K_MER = 16                          # Indexer: k-mer length (indexer.rs; oracle/indexer_model.py K)
VOTE_GATE = 20                      # map_read's gate: 2 * count1 >= 40 (indexer.rs:353-360)
MERGE_MIN_OVERLAP = 30              # fast_merge: the smallest overlap it tries (read.rs:313-440)
# a read of L bases has L - K_MER + 1 windows, each votes at most once per diagonal: a 30-mer cannot pass the gate
SE_FILLER_LEN = 30
assert SE_FILLER_LEN - K_MER + 1 < VOTE_GATE
# a pair merges only with an overlap of MERGE_MIN_OVERLAP bases or more, which neither read may be shorter than: the
# pair filler is one base short of that (and passes the vote gate even less than a 30-mer)
MC_FILLER_LEN = MERGE_MIN_OVERLAP - 1
FILLER_POOL = 256

BOUNDARY_THREADS = (1, 2, WAVE - 1, WAVE, WAVE + 1, SCAN_THREADS // 2 - 1, SCAN_THREADS // 2, SCAN_THREADS - 1)
RANDOM_TILES = 300
FILL = 0xEE


def rc_tile() -> int:
    from genefuserust_amd.ref_cut import tile_bytes
    return tile_bytes()


TAILS = {SE_TILE: (SE_PER + 1, SE_TILE // 2 + 3), MC_TILE: (5, MC_TILE // 2 + 1)}   # the partial last tiles


def batch_sizes(T: int) -> dict:
    """a: the smallest batch that crosses wavefront 0 of the scan block (per = 1).  b: runs of two tiles, with threads
    left over; its tiles make whole runs, so c is one tile less: the last run is shorter than per."""
    half = SCAN_THREADS // 2
    return {"a": (WAVE + 1) * T + TAILS[T][0], "b": (SCAN_THREADS + half + 1) * T + TAILS[T][1],
            "c": (SCAN_THREADS + half) * T + TAILS[T][1]}


def scan_shape(n: int, T: int = 1) -> Tuple[int, int, int, int]:
    """(tiles, per, threads that have a run, length of the last run) of the one-block scan over ceil(n / T) totals."""
    ntiles = -(-n // T)
    per = max(-(-ntiles // SCAN_THREADS), 1)
    busy = -(-ntiles // per)
    return ntiles, per, busy, ntiles - (busy - 1) * per


# ---- 0. the sizes are the sources' ---------------------------------------------------------------------------------

def _define(header: str, name: str) -> str:
    src = open(os.path.join(SCAN_CSRC, header)).read()
    m = re.search(r"^#define\s+%s\s+(.+?)\s*(?://.*)?$" % name, src, flags=re.M)
    assert m, (header, name)
    return m.group(1)


def test_sizes_are_the_sources_defines():
    assert int(_define("gf_scan_common.h", "GF_SCAN_THREADS")) == BLOCK
    assert int(_define("gf_scan_common.h", "GF_SCAN_TOTALS_THREADS")) == SCAN_THREADS
    assert int(_define("gf_se_kernels.h", "GF_SE_PER")) == SE_PER
    assert _define("gf_se_kernels.h", "GF_SE_TILE") == "(GF_SCAN_THREADS * GF_SE_PER)"
    assert _define("gf_mc_kernels.h", "GF_MC_TILE") == "GF_SCAN_THREADS"
    assert int(_define("gf_rc_kernels.h", "GF_RC_PIECE")) == RC_PIECE
    assert _define("gf_rc_kernels.h", "GF_RC_THREADS") == "GF_SCAN_THREADS"
    assert _define("gf_rc_kernels.h", "GF_RC_TILE") == "(GF_RC_THREADS * GF_RC_PIECE)"
    assert rc_tile() == BLOCK * RC_PIECE
    # the names' grids: gf_hn_k_lengths a thread per record up to HN_GRID_BLOCKS blocks, then it strides
    src = open(os.path.join(SCAN_CSRC, "gf_hit_names.hip")).read()
    m = re.search(r"g_len\s*=.*?\(hits_cap \+ GF_SCAN_THREADS - 1\) / GF_SCAN_THREADS,\s*(\d+)\)", src)
    assert m and int(m.group(1)) == HN_GRID_BLOCKS
    # the split of the totals is written once, in the shared body, and every scan kernel is still its library's own
    split = r"per = \((?:ntiles|n) \+ GF_SCAN_TOTALS_THREADS - 1\) / GF_SCAN_TOTALS_THREADS;"
    assert len(re.findall(split, open(os.path.join(SCAN_CSRC, "gf_scan_common.h")).read())) == 1
    for header, kernels in (("gf_se_kernels.h", ("gf_se_k_scan",)), ("gf_mc_kernels.h", ("gf_mc_k_scan",)),
                            ("gf_hn_kernels.h", ("gf_hn_k_scan",)),
                            ("gf_rc_kernels.h", ("gf_rc_k_scan", "gf_rc_k_name_scan"))):
        src = open(os.path.join(SCAN_CSRC, header)).read()
        assert not re.findall(split, src), header
        for kernel in kernels:
            assert len(re.findall(r"__global__[^;{]*?\bvoid %s\(" % kernel, src)) == 1, kernel


def test_batch_sizes_cross_the_thresholds():
    for T in (SE_TILE, MC_TILE):
        s = batch_sizes(T)
        ntiles, per, busy, last = scan_shape(s["a"], T)
        assert per == 1 and WAVE < ntiles <= 2 * WAVE and s["a"] % T != 0        # the second wavefront, a partial tile
        assert scan_shape(WAVE * T, T)[0] == WAVE                                # (one tile less stays in wavefront 0)
        ntiles, per, busy, last = scan_shape(s["b"], T)
        assert per == 2 and busy < SCAN_THREADS and s["b"] % T != 0
        ntiles, per, busy, last = scan_shape(s["c"], T)
        assert per == 2 and last < per and busy < SCAN_THREADS and s["c"] % T != 0
    for count, per, last in ((SCAN_THREADS + 1, 2, 1), (2 * SCAN_THREADS + 1, 3, 3), (2 * SCAN_THREADS + 2, 3, 1),
                             (3 * SCAN_THREADS + 1, 4, 1)):
        assert scan_shape(count)[1::2] == (per, last) and scan_shape(count)[2] < SCAN_THREADS


# ---- 1. planted elements, their outcome by the oracle chain, and the expectation builder -------------------------------

class Hit(NamedTuple):
    source: int
    flags: int            # bit 0: found on the reverse complement; bit 1: ReadMatch.m_reversed
    seq: bytes            # as the record's bytes hold it (reverse-complemented on the retry)
    qual: bytes
    merge_diff: int
    m: tuple              # ((seq_start, seq_end, contig, position),) * 2 of the oracle's map_read


class Outcome(NamedTuple):
    retried: int          # candidates that were searched again as their reverse complement
    merged: int           # 1: the pair merged
    hits: Tuple[Hit, ...]


def _one(oracle, ox, rev, seq: bytes, qual: bytes, source: int):
    """sescanner.rs:183-205 / pescanner.rs:465-511 for one candidate read: (retried, [Hit])."""
    st, _ = oracle.fusion_map_read(ox, rev, seq, ox.map_read(seq))
    if st == 2:
        return 0, [Hit(source, 0, seq, qual, 0, tuple(ox.map_read(seq)))]
    if st == 1:   # mapable, no match: the reverse complement
        s2, q2 = rc(seq), qual[::-1]
        st, _ = oracle.fusion_map_read(ox, rev, s2, ox.map_read(s2))
        if st == 2:
            return 1, [Hit(source, 1 | (2 if source else 0), s2, q2, 0, tuple(ox.map_read(s2)))]
        return 1, []
    return 0, []


def read_outcome(oracle, ox, rev, read: bytes, qual: bytes) -> Outcome:
    r, h = _one(oracle, ox, rev, read, qual, 1)
    return Outcome(r, 0, tuple(h))


def pair_outcome(oracle, ox, rev, pair) -> Outcome:
    s1, q1, s2, q2 = pair
    m = oracle.fast_merge(s1, q1, s2, q2)
    if m is not None:
        r, h = _one(oracle, ox, rev, m[0], m[1], 0)
        return Outcome(r, 1, tuple(x._replace(merge_diff=m[2]) for x in h))
    r1, h1 = _one(oracle, ox, rev, s1, q1, 1)
    r2, h2 = _one(oracle, ox, rev, s2, q2, 2)
    return Outcome(r1 + r2, 0, tuple(h1 + h2))


NOTHING = Outcome(0, 0, ())


def expected_scan(positions, elems, outcomes, base: int = 0, forward_only: bool = False):
    """The scan of a batch whose elements give nothing but for element ``elems[j]`` at ``positions[j]``: (records as
    PAIR_HIT_DTYPE, hit bases, hit qualities, totals).  ``forward_only``: what an emptied retry pass leaves."""
    from genefuserust_amd import _lib
    rows, hb, hq, off, retried, merged = [], [], [], 0, 0, 0
    for j in np.argsort(np.asarray(positions), kind="stable"):
        o = outcomes[elems[j]]
        retried += o.retried
        merged += o.merged
        for h in o.hits:
            if forward_only and h.flags & 1:
                continue
            rows.append((base + int(positions[j]), h, off))
            hb.append(h.seq)
            hq.append(h.qual)
            off += len(h.seq)
    rec = np.zeros(len(rows), dtype=_lib.PAIR_HIT_DTYPE)
    for k, (pid, h, o) in enumerate(rows):
        rec[k]["pair_id"], rec[k]["source"], rec[k]["flags"], rec[k]["read_len"] = pid, h.source, h.flags, len(h.seq)
        rec[k]["merge_diff"], rec[k]["seq_offset"] = h.merge_diff, o
        for i, (ss, se, contig, pos) in enumerate(h.m):
            rec[k]["m"][i] = (ss, se, pos, contig, 0)
    return rec, b"".join(hb), b"".join(hq), {"hits": len(rows), "hit_bytes": off, "merged_pairs": merged,
                                             "retried_reads": retried, "overflow": 0, "too_long": 0}


FIELDS = ("pair_id", "source", "flags", "read_len", "merge_diff", "seq_offset")
M_FIELDS = ("seq_start", "seq_end", "contig", "position")


def assert_scan(got, want, what=""):
    """(records, bases, qualities, totals) field by field and byte by byte; the totals over the keys ``got`` has."""
    (gr, gb, gq, gt), (wr, wb, wq, wt) = got, want
    assert gt == {k: wt[k] for k in gt}, (what, gt, wt)
    assert gr.shape == wr.shape, what
    for f in FIELDS:
        bad = np.flatnonzero(gr[f] != wr[f])
        assert bad.size == 0, (what, f, int(bad[0]), int(gr[f][bad[0]]), int(wr[f][bad[0]]))
    for f in M_FIELDS:
        bad = np.flatnonzero((gr["m"][f] != wr["m"][f]).any(axis=1)) if len(gr) else np.zeros(0, int)
        assert bad.size == 0, (what, "m." + f, int(bad[0]))
    assert gb == wb and gq == wq, what


def _quals(rng, reads):
    return [bytes(rng.integers(33, 75, size=len(r), dtype=np.uint8)) for r in reads]


def _pick(outcomes, marks, limit=64, per_kind=5):
    """Indices of up to ``limit`` elements, at most ``per_kind`` of each kind (what the outcome is, and the mark)."""
    seen, out = {}, []
    for i, (o, mk) in enumerate(zip(outcomes, marks)):
        kind = (o.retried, o.merged, tuple((h.source, h.flags) for h in o.hits), mk)
        if seen.get(kind, 0) < per_kind and len(out) < limit:
            seen[kind] = seen.get(kind, 0) + 1
            out.append(i)
    return out


def _mark(seq: bytes) -> str:
    if not seq:
        return "empty"
    if seq != seq.upper():
        return "lower"
    return "iupac" if set(seq) - set(b"ACGT") else "plain"


class Pool(NamedTuple):
    genes: list
    rev: list
    elems: list           # reads (bytes) or pairs (s1, q1, s2, q2)
    quals: list           # single-end: the reads' qualities
    outcomes: list
    retry: list           # indices of elements that use a retry slot
    forward: list         # indices of elements that are a hit as they are, nothing retried


def _kinds(outcomes):
    retry = [i for i, o in enumerate(outcomes) if o.retried]
    forward = [i for i, o in enumerate(outcomes) if not o.retried and o.hits and all(h.flags == 0 for h in o.hits)]
    return retry, forward


@pytest.fixture(scope="module")
def se_pool(oracle) -> Pool:
    """About 64 distinct reads of tests/test_single_end_device.py's generator, and four junctions of one gene with
    itself across strands (two segments that are in the required direction on neither strand)."""
    from tests.test_single_end_device import _synthetic
    genes, rev, reads = _synthetic(n_reads=1200, seed=21)
    rng = np.random.default_rng(2)
    for k in range(4):
        g = genes[k]
        a, b = int(rng.integers(0, 1000)), int(rng.integers(1500, 2500))
        reads.append(g[a:a + 75] + rc(g[b:b + 75]))
    reads += [b"", genes[0][100:130]]
    reads = list(dict.fromkeys(reads))
    quals = _quals(rng, reads)
    ox = oracle.OracleIndexer(genes)
    outcomes = [read_outcome(oracle, ox, rev, r, q) for r, q in zip(reads, quals)]
    keep = _pick(outcomes[::-1], [_mark(r) for r in reads[::-1]], per_kind=8)     # (from the end: the crafted reads are in)
    keep = [len(reads) - 1 - i for i in keep]
    reads, quals, outcomes = [reads[i] for i in keep], [quals[i] for i in keep], [outcomes[i] for i in keep]
    return Pool(genes, rev, reads, quals, outcomes, *_kinds(outcomes))


def test_single_end_pool_holds_every_kind(se_pool):
    o = se_pool.outcomes
    assert 40 <= len(o) <= 64 and len(set(se_pool.elems)) == len(o)
    assert sum(1 for x in o if x.hits and x.hits[0].flags == 0) >= 5           # forward hits
    assert sum(1 for x in o if x.hits and x.hits[0].flags == 3) >= 5           # retries that hit on the other strand
    assert sum(1 for x in o if x.retried and not x.hits) >= 2                  # two segments, a hit on neither strand
    assert sum(1 for x in o if not x.retried and not x.hits) >= 5              # nothing
    marks = {_mark(r) for r in se_pool.elems}
    assert marks == {"empty", "lower", "iupac", "plain"}
    hit_marks = {_mark(r) for r, x in zip(se_pool.elems, o) if x.hits}
    assert "iupac" in hit_marks and "plain" in hit_marks


def _golden_sets():
    from tests.test_multi_csv_scan import _gene_sets
    (genes, rev), (other, _) = _gene_sets(np.random.default_rng(5))[:2]
    return [(genes, rev), (other, [bool(i % 2) for i in range(len(other))])]


@pytest.fixture(scope="module")
def mc_pool(oracle):
    """About 64 distinct pairs of tests/test_multi_csv_scan.py's pair maker, and four whose merged read is a junction of
    one gene with itself across strands; their outcomes against two gene sets with different reversed flags."""
    from tests.test_multi_csv_scan import _make_pairs, _ragged
    sets = _golden_sets()
    genes = sets[0][0]
    rng = np.random.default_rng(5)
    pairs = _ragged(rng, _make_pairs(rng, genes, 780))
    for k in range(4):
        g = genes[k % 3]
        a, b = int(rng.integers(0, 600)), int(rng.integers(900, 1500))
        f = g[a:a + 100] + rc(g[b:b + 100])
        pairs.append((f[:150], b"F" * 150, rc(f)[:150], b"F" * 150))
    pairs = list(dict.fromkeys(pairs))
    ox = oracle.OracleIndexer(genes)
    outcomes = [pair_outcome(oracle, ox, sets[0][1], p) for p in pairs]
    marks = [_mark(p[0]) + "/" + _mark(p[2]) for p in pairs]
    keep = [len(pairs) - 1 - i for i in _pick(outcomes[::-1], marks[::-1], per_kind=3)]
    pairs = [pairs[i] for i in keep]
    pools = []
    for seqs, rev in sets:
        ox = oracle.OracleIndexer(seqs)
        out = [pair_outcome(oracle, ox, rev, p) for p in pairs]
        pools.append(Pool(seqs, rev, pairs, [], out, *_kinds(out)))
    return pools


def test_pair_pool_holds_every_kind(mc_pool):
    assert mc_pool[0].rev != mc_pool[1].rev
    for pool in mc_pool:
        o = pool.outcomes
        assert 40 <= len(o) <= 64 and len(set(pool.elems)) == len(o)
        assert sum(x.merged for x in o) >= 8 and sum(1 - x.merged for x in o) >= 8
        assert {h.source for x in o for h in x.hits} == {0, 1, 2}
        assert {h.flags for x in o for h in x.hits} == {0, 1, 3}
        assert sum(1 for x in o if x.retried and not x.hits) >= 1 and sum(1 for x in o if x.retried > len(x.hits)) >= 1
        assert pool.retry and pool.forward
    assert [x.merged for x in mc_pool[0].outcomes] == [x.merged for x in mc_pool[1].outcomes]
    assert mc_pool[0].outcomes != mc_pool[1].outcomes
    marks = {_mark(s) for p in mc_pool[0].elems for s in (p[0], p[2])}
    assert marks >= {"empty", "lower", "iupac", "plain"}


def filler_pool(length: int, seed: int = 77):
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(0, 4, size=(2 * FILLER_POOL, length)), axis=0)
    pool = pool[rng.permutation(pool.shape[0])[:FILLER_POOL]]
    assert pool.shape == (FILLER_POOL, length)
    return np.frombuffer(b"ACGT", dtype=np.uint8)[pool]


def placement(n: int, T: int, seed: int, inner: bool = False):
    """Where the planted elements go: [(position, kind)], kind "retry" / "hit" / "any", positions distinct.  Both sides
    of the run boundaries of BOUNDARY_THREADS and of the last tile get a retry followed by a hit, so that an offset
    that is wrong there shifts a slot; the corners; and one element in RANDOM_TILES further tiles spread over the runs
    of all wavefronts of the scan block (``inner``: thread and wavefront boundaries inside the tile too)."""
    ntiles, per, busy, last = scan_shape(n, T)
    rng = np.random.default_rng(seed)
    at = {}

    def put(p, kind):
        if 0 <= p < n:
            at.setdefault(int(p), kind)

    for t in sorted({per * k for k in BOUNDARY_THREADS if per * k < ntiles} | {ntiles - 1}):
        for p, kind in ((t * T - 2, "retry"), (t * T - 1, "hit"), (t * T, "retry"), (t * T + 1, "hit")):
            put(p, kind)
    for p in (0, n - 1, (ntiles - 1) * T):
        put(p, "any")
    tiles = []
    waves = [range(WAVE * w * per, min(WAVE * (w + 1) * per, ntiles)) for w in range(SCAN_THREADS // WAVE)]
    waves = [w for w in waves if len(w)]
    for w in waves:
        want = min(len(w), -(-RANDOM_TILES // len(waves)) + 2)   # (the last wavefront's runs may be few)
        tiles += [int(t) for t in rng.choice(np.arange(w.start, w.stop), size=want, replace=False)]
    for j, t in enumerate(tiles):
        room = min(T, n - t * T)
        put(t * T + int(rng.integers(0, room)), "any")
        if inner and j % 8 == 0:   # thread boundaries 16k - 1 | 16k and wavefront boundaries 1024k - 1 | 1024k
            k, w = int(rng.integers(1, BLOCK)), int(rng.integers(1, BLOCK // WAVE))
            for p in (SE_PER * k - 1, SE_PER * k, WAVE * SE_PER * w - 1, WAVE * SE_PER * w):
                if p < room:
                    put(t * T + p, "any")
    return sorted(at.items()), len(set(tiles))


def plant(pool: Pool, places):
    """Which element of the pool goes to each place: retries and hits where the place asks for one, else every element
    of the pool in turn."""
    positions, elems, turn = [], [], {"retry": 0, "hit": 0, "any": 0}
    for p, kind in places:
        src = {"retry": pool.retry, "hit": pool.forward, "any": range(len(pool.elems))}[kind]
        positions.append(p)
        elems.append(src[turn[kind] % len(src)])
        turn[kind] += 1
    return np.array(positions, dtype=np.int64), elems


def ragged_with_filler(n: int, positions, seqs, quals, filler=None, seed: int = 3):
    """bases, qualities, offsets of n reads: ``seqs[j]`` at ``positions[j]`` (ascending), every other read empty, or a
    row of ``filler`` drawn with ``seed``."""
    flen = 0 if filler is None else filler.shape[1]
    lens = np.full(n, flen, dtype=np.int64)
    lens[positions] = [len(s) for s in seqs]
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    b = np.empty(int(off[-1]), dtype=np.uint8)
    q = np.full(int(off[-1]), ord("I"), dtype=np.uint8)
    if filler is not None:
        draw = np.random.default_rng(seed).integers(0, filler.shape[0], size=n)
        prev = 0
        for p in list(positions) + [n]:
            if p > prev:
                b[off[prev]:off[p]] = filler[draw[prev:p]].reshape(-1)
            prev = p + 1
    for p, s, ql in zip(positions, seqs, quals):
        b[off[p]:off[p] + len(s)] = np.frombuffer(s, dtype=np.uint8)
        q[off[p]:off[p] + len(s)] = np.frombuffer(ql, dtype=np.uint8)
    return b, q, off


def _read_at(b, q, off, p):
    return b[off[p]:off[p + 1]].tobytes(), q[off[p]:off[p + 1]].tobytes()


def test_builder_equals_the_policy_on_every_position(oracle, se_pool, mc_pool):
    """10 000 positions, 200 planted, the rest empty or a filler: the policy over the oracle on EVERY position, fillers
    included, gives what the builder gives from the planted ones alone."""
    n, planted = 10_000, 200
    rng = np.random.default_rng(8)
    positions = np.sort(rng.choice(n, size=planted, replace=False))
    kinds = [("retry", "hit", "any")[int(k)] for k in rng.integers(0, 3, size=planted)]
    # single-end
    pos, elems = plant(se_pool, list(zip(positions.tolist(), kinds)))
    ox = oracle.OracleIndexer(se_pool.genes)
    for filler in (None, filler_pool(SE_FILLER_LEN)):
        b, q, off = ragged_with_filler(n, pos, [se_pool.elems[e] for e in elems], [se_pool.quals[e] for e in elems], filler)
        every = [read_outcome(oracle, ox, se_pool.rev, *_read_at(b, q, off, p)) for p in range(n)]
        want = expected_scan(np.arange(n), list(range(n)), every, base=7)
        got = expected_scan(pos, elems, se_pool.outcomes, base=7)
        assert_scan(got, want)
        assert got[3]["hits"] >= 50 and got[3]["retried_reads"] >= 50 and got[0]["flags"].tolist().count(3) >= 20
    # pairs
    pool = mc_pool[0]
    pos, elems = plant(pool, list(zip(positions.tolist(), kinds)))
    ox = oracle.OracleIndexer(pool.genes)
    for filler in (None, filler_pool(MC_FILLER_LEN)):
        sides = [ragged_with_filler(n, pos, [pool.elems[e][s] for e in elems], [pool.elems[e][s + 1] for e in elems],
                                    filler, seed=3 + s) for s in (0, 2)]
        every = [pair_outcome(oracle, ox, pool.rev, _read_at(*sides[0], p) + _read_at(*sides[1], p)) for p in range(n)]
        want = expected_scan(np.arange(n), list(range(n)), every, base=7)
        got = expected_scan(pos, elems, pool.outcomes, base=7)
        assert_scan(got, want)
        assert got[3]["merged_pairs"] >= 20 and {int(s) for s in got[0]["source"]} == {0, 1, 2}


def test_fillers_give_nothing(oracle, se_pool, mc_pool):
    """No filler maps against any of the gene sets, and no two fillers merge."""
    se, mc = filler_pool(SE_FILLER_LEN), filler_pool(MC_FILLER_LEN)
    assert len({r.tobytes() for r in se}) == FILLER_POOL == len({r.tobytes() for r in mc})
    for genes in (se_pool.genes, mc_pool[0].genes, mc_pool[1].genes):
        ox = oracle.OracleIndexer(genes)
        for r in [b""] + [x.tobytes() for x in se] + [x.tobytes() for x in mc]:
            assert ox.map_read(r) == [] and ox.map_read(rc(r)) == []
    assert read_outcome(oracle, oracle.OracleIndexer(se_pool.genes), se_pool.rev, b"", b"") == NOTHING
    qual = b"I" * MC_FILLER_LEN
    assert oracle.fast_merge(b"", b"", b"", b"") is None
    for k in range(FILLER_POOL):   # every filler against its own reverse complement (the one overlap there could be) ..
        assert oracle.fast_merge(mc[k].tobytes(), qual, rc(mc[k].tobytes()), qual) is None
    rng = np.random.default_rng(1)   # .. and random pairs of them, either way round
    for a, b in rng.integers(0, FILLER_POOL, size=(2000, 2)):
        assert oracle.fast_merge(mc[a].tobytes(), qual, mc[b].tobytes(), qual) is None
        assert oracle.fast_merge(mc[a].tobytes(), qual, rc(mc[b].tobytes()), qual) is None


def test_placement_reaches_every_level():
    for T, inner in ((SE_TILE, True), (MC_TILE, False)):
        for name, n in batch_sizes(T).items():
            ntiles, per, busy, last = scan_shape(n, T)
            places, n_random = placement(n, T, seed=11, inner=inner)
            pos = np.array([p for p, _ in places])
            assert len(set(pos.tolist())) == len(pos) and pos.min() == 0 and pos.max() == n - 1
            assert (ntiles - 1) * T in pos
            tiles = np.unique(pos // T)
            assert n_random >= min(RANDOM_TILES, ntiles)
            owners = np.unique(tiles // per // WAVE)                               # wavefronts of the scan block
            assert owners.tolist() == list(range(-(-busy // WAVE)))
            for k in BOUNDARY_THREADS:
                if per * k < ntiles:
                    assert {per * k * T - 2, per * k * T - 1, per * k * T, per * k * T + 1} <= set(pos.tolist())
            if per > 1:   # positions inside a run, behind its first tile
                assert (tiles % per != 0).sum() >= 100
            if inner:
                inside = pos % T
                assert ((inside % SE_PER == SE_PER - 1).sum() >= 10 and (inside % SE_PER == 0).sum() >= 10
                        and (inside % (WAVE * SE_PER) == 0).sum() >= 10)


# ---- 2. single-end: gf_se_scan_device ----------------------------------------------------------------------------------

def _cuda(*arrays):
    import torch
    return [torch.from_numpy(a).cuda() for a in arrays]


@pytest.fixture(scope="module")
def se_index(gpu_device, se_pool):
    from genefuserust_amd import Indexer
    ix = Indexer.from_gene_slices(se_pool.genes, se_pool.rev)
    ix.make_index()
    yield ix
    ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size,filler", [("a", "empty"), ("b", "empty"), ("b", "30-mers"), ("c", "empty")])
def test_single_end_scan_past_one_tile_per_scan_thread(se_index, se_pool, size, filler):
    from genefuserust_amd.single_end import scan_single_device
    n = batch_sizes(SE_TILE)[size]
    places, _ = placement(n, SE_TILE, seed=11, inner=True)
    pos, elems = plant(se_pool, places)
    b, q, off = ragged_with_filler(n, pos, [se_pool.elems[e] for e in elems], [se_pool.quals[e] for e in elems],
                                   filler_pool(SE_FILLER_LEN) if filler != "empty" else None)
    db, dq, doff = _cuda(b, q, off)
    max_len = 300
    want = expected_scan(pos, elems, se_pool.outcomes)
    tot = want[3]
    n_retry, n_hits = tot["retried_reads"], tot["hits"]
    assert n_hits >= 30 and n_retry >= 30 and tot["hits"] > (want[0]["flags"] == 0).sum() > 10
    room = dict(hits_cap=n_hits + 16, bytes_cap=tot["hit_bytes"] + 64)

    def run(**kw):
        scan = scan_single_device(se_index, db, dq, doff, max_len, **{**room, **kw})
        got = scan.download()
        got[3]["too_long"] = int(scan.totals[5].item())
        got[3].pop("merged_pairs")
        return got

    assert_scan(run(retry_cap=n_retry + 100), want, "room")
    # as many retry slots as retries: the same; one fewer: bit 1, the retry pass emptied, the hits on the reads as they are
    assert_scan(run(retry_cap=n_retry), want, "retry_cap == retries")
    fwd = expected_scan(pos, elems, se_pool.outcomes, forward_only=True)
    fwd[3]["overflow"] = 1
    assert_scan(run(retry_cap=n_retry - 1), fwd, "retry_cap one short")
    # one record fewer than hits: bit 2, the true totals, the records that fit
    rec, hb, hq, t = run(retry_cap=n_retry, hits_cap=n_hits - 1)
    assert t == {**{k: tot[k] for k in t}, "overflow": 2}
    assert_scan((rec, hb, hq, {}), (want[0][:n_hits - 1], want[1], want[2], {}), "hits_cap one short")
    # read_id_base shifts pair_id and nothing else
    base = (1 << 32) + 12345
    assert_scan(run(retry_cap=n_retry, read_id_base=base), expected_scan(pos, elems, se_pool.outcomes, base=base), "base")


# ---- 3. multi-CSV: gf_mc_pairs_prepare_device + gf_mc_pairs_scan_device ------------------------------------------------

def _take(off, nbytes):
    """gf_scan_host.h: buffers are carved in 256-byte aligned pieces."""
    return off + ((nbytes + 255) & ~255)


def prepared_parts(prepared, n: int, l_bytes: int, r_bytes: int):
    """The lists of a prepared buffer (prepared_layout of gf_multi_csv.hip, restated): header, merged lengths and
    diffs, the unmerged list's offsets, the merged list's, the lists' bases and the merged reads' qualities."""
    import torch
    pad = (-prepared.buffer.data_ptr()) % 256
    host = prepared.buffer[pad:].cpu().numpy()
    cap = l_bytes + r_bytes
    o_hdr = 0
    o_mlen = _take(o_hdr, 256)
    o_mdiff = _take(o_mlen, 4 * n)
    o_rank = _take(o_mdiff, 4 * n)
    o_mpos = _take(o_rank, 4 * n)
    o_uoff = _take(o_mpos, 8 * n)
    o_moff = _take(o_uoff, 8 * (2 * n + 1))
    o_bases = _take(o_moff, 8 * (n + 1))
    o_mq = _take(o_bases, cap + 64)
    view = lambda o, count, dt: host[o:o + count * np.dtype(dt).itemsize].view(dt)
    return {"hdr": view(o_hdr, 4, np.int64), "m_len": view(o_mlen, n, np.int32), "m_diff": view(o_mdiff, n, np.int32),
            "u_off": view(o_uoff, 2 * n + 1, np.int64), "m_off": view(o_moff, n + 1, np.int64),
            "bases": host[o_bases:o_bases + cap], "m_quals": host[o_mq:o_mq + cap]}


def expected_prepared(oracle, n, positions, pairs, sides):
    """The same lists from which planted pairs oracle.fast_merge merges (no filler pair does): the unmerged list is R1
    then R2 of every unmerged pair in pair order, the merged list the merged reads in pair order, behind it."""
    (lb, _, lo), (rb, _, ro) = sides
    m_len, m_diff = np.zeros(n, np.int32), np.zeros(n, np.int32)
    mseq, mqual = [], []
    for p, pair in zip(positions, pairs):
        m = oracle.fast_merge(*pair)
        if m is not None:
            m_len[p], m_diff[p] = len(m[0]), m[2]
            mseq.append(m[0])
            mqual.append(m[1])
    un = m_len == 0
    nu, nm = int(un.sum()), n - int(un.sum())
    lens = np.stack([np.diff(lo)[un], np.diff(ro)[un]], axis=1).reshape(-1)
    ub = int(lens.sum())
    u_off = np.full(2 * n + 1, ub, dtype=np.int64)
    u_off[0] = 0
    np.cumsum(lens, out=u_off[1:2 * nu + 1])
    mb = int(m_len.sum())
    m_off = np.full(n + 1, ub + mb, dtype=np.int64)
    m_off[:nm] = ub + np.concatenate([[0], np.cumsum(m_len[~un])[:-1]]) if nm else m_off[:nm]
    # the unmerged bytes: every read of both sides but the merged pairs', interleaved pair by pair
    ubytes = np.empty(ub, dtype=np.uint8)
    lkeep, rkeep = np.repeat(un, np.diff(lo)), np.repeat(un, np.diff(ro))
    l_dst = np.repeat(u_off[0:2 * nu:2] - lo[:-1][un], np.diff(lo)[un]) + np.flatnonzero(lkeep)
    r_dst = np.repeat(u_off[1:2 * nu:2] - ro[:-1][un], np.diff(ro)[un]) + np.flatnonzero(rkeep)
    ubytes[l_dst] = lb[lkeep]
    ubytes[r_dst] = rb[rkeep]
    return {"hdr": np.array([nu, ub, nm, mb]), "m_len": m_len, "m_diff": m_diff, "u_off": u_off, "m_off": m_off,
            "bases": np.concatenate([ubytes, np.frombuffer(b"".join(mseq), dtype=np.uint8)]),
            "m_quals": np.frombuffer(b"".join(mqual), dtype=np.uint8), "ub": ub}


@pytest.fixture(scope="module")
def mc_indexes(gpu_device, mc_pool):
    from genefuserust_amd import Indexer
    out = []
    for pool in mc_pool:
        ix = Indexer.from_gene_slices(pool.genes, pool.rev)
        ix.make_index()
        out.append(ix)
    yield out
    for ix in out:
        ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size,filler", [("a", "empty"), ("b", "empty"), ("b", "29-mers"), ("c", "empty")])
def test_multi_csv_scan_past_one_tile_per_scan_thread(mc_indexes, mc_pool, oracle, size, filler):
    from genefuserust_amd.multi_csv_scan import prepare_pairs_device, scan_prepared_pairs_device
    from genefuserust_amd.read_pair import scan_pairs_device
    from tests.test_multi_csv_scan import _same
    n = batch_sizes(MC_TILE)[size]
    places, _ = placement(n, MC_TILE, seed=12)
    pos, elems = plant(mc_pool[0], places)
    pairs = [mc_pool[0].elems[e] for e in elems]
    fill = filler_pool(MC_FILLER_LEN) if filler != "empty" else None
    sides = [ragged_with_filler(n, pos, [p[s] for p in pairs], [p[s + 1] for p in pairs], fill, seed=3 + s) for s in (0, 2)]
    t = _cuda(*sides[0]) + _cuda(*sides[1])
    max_len = 150
    # ONE prepared buffer, made with the first index: its lists against the restatement
    prepared = prepare_pairs_device(mc_indexes[0], *t, max_len)
    got_p = prepared_parts(prepared, n, sides[0][0].size, sides[1][0].size)
    want_p = expected_prepared(oracle, n, pos, pairs, sides)
    ub, mb = want_p["ub"], int(want_p["hdr"][3])
    assert want_p["hdr"][2] >= 15 and got_p["hdr"].tolist() == want_p["hdr"].tolist()
    assert (np.maximum(got_p["m_len"], 0) == want_p["m_len"]).all()
    merged = want_p["m_len"] > 0
    assert (got_p["m_diff"][merged] == want_p["m_diff"][merged]).all()
    assert (got_p["u_off"] == want_p["u_off"]).all() and (got_p["m_off"] == want_p["m_off"]).all()
    assert (got_p["bases"][:ub + mb] == want_p["bases"]).all()
    assert (got_p["m_quals"][ub:ub + mb] == want_p["m_quals"]).all()
    assert prepared.merged_pairs() == int(want_p["hdr"][2])
    for ix, pool in zip(mc_indexes, mc_pool):
        want = expected_scan(pos, elems, pool.outcomes, base=1000)
        tot = want[3]
        n_retry, n_hits = tot["retried_reads"], tot["hits"]
        assert n_hits >= 30 and n_retry >= 30 and {int(s) for s in want[0]["source"]} == {0, 1, 2}
        room = dict(hits_cap=n_hits + 16, bytes_cap=tot["hit_bytes"] + 64, pair_id_base=1000)

        def run(**kw):
            return scan_prepared_pairs_device(ix, prepared, **{**room, **kw}).download()

        got = run(retry_cap=n_retry + 100)
        assert_scan(got, want, "room")
        # the second, independent check: the one-call scan on the same batch, every byte of the records
        _same(got, scan_pairs_device(ix, *t, max_len, retry_cap=n_retry + 100, **room).download())
        assert_scan(run(retry_cap=n_retry), want, "retry_cap == retries")
        fwd = expected_scan(pos, elems, pool.outcomes, base=1000, forward_only=True)
        fwd[3]["overflow"] = 1
        assert_scan(run(retry_cap=n_retry - 1), fwd, "retry_cap one short")
        rec, hb, hq, tt = run(retry_cap=n_retry, hits_cap=n_hits - 1)
        assert tt == {**{k: tot[k] for k in tt}, "overflow": 2}
        assert_scan((rec, hb, hq, {}), (want[0][:n_hits - 1], want[1], want[2], {}), "hits_cap one short")


# ---- 4. hit names: gf_hn_names_device -------------------------------------------------------------------------------

HN_RECORDS = 6000
HN_BASE = 5_000_000_000


def _name_lines(rng, step: int, shift: int):
    """HN_RECORDS name lines of 0 .. 200 bytes: the copy's 64-byte steps run one, two, three and four rounds."""
    out = []
    for i in range(HN_RECORDS):
        ln = (i * step + shift) % 201
        out.append((b"@" + bytes(rng.integers(48, 123, size=ln, dtype=np.uint8)))[:ln])
    return out


@pytest.fixture(scope="module")
def hn_texts(gpu_device):
    """A FASTQ text pair of HN_RECORDS records, cut on the device: R2's names differ from R1's, and neither text ends
    in a newline."""
    import torch
    from genefuserust_amd import Indexer
    from genefuserust_amd.fastq import fastq_cut_device
    rng = np.random.default_rng(6)
    names = [_name_lines(rng, 7, 5), _name_lines(rng, 11, 3)]
    assert names[0] != names[1] and {len(x) for x in names[0]} == set(range(201)) == {len(x) for x in names[1]}
    texts = [b"\n".join(nm + b"\nACGTACGT\n+\nFFFFFFFF" for nm in side) for side in names]
    ix = Indexer.from_gene_slices([rand_seq(rng, 400)])
    ix.make_index()
    dev = [torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda() for t in texts]
    batches = [fastq_cut_device(ix, d) for d in dev]
    assert [b.n_records for b in batches] == [HN_RECORDS] * 2
    assert [b.n_newlines for b in batches] == [4 * HN_RECORDS - 1] * 2
    yield ix, names, dev, batches
    ix.close()


def _hn_records(count: int, seed: int):
    """``count`` gf_pair_hit records naming arbitrary (record, source) pairs, repeats among them, in no order; every
    500th names a record off the text.  -> (records, the names they have to get, how many have none)."""
    from genefuserust_amd import _lib
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, HN_RECORDS, size=count)
    src = rng.integers(0, 3, size=count)
    off_text = np.arange(17, count, 500)
    ids[off_text] = np.resize(np.array([HN_RECORDS, HN_RECORDS + 1, 10 ** 9, -1, -HN_BASE - 5]), off_text.size)
    rec = np.zeros(count, dtype=_lib.PAIR_HIT_DTYPE)
    rec["pair_id"], rec["source"] = ids + HN_BASE, src
    return rec, ids, src, int(off_text.size)


def _hn_call(hn_texts, rec, hits_cap: int, names_cap: int, guard: int = 0):
    """gf_hn_names_device over ``rec`` in a record buffer of ``hits_cap``; the names' buffer holds FILL and is ``guard``
    bytes longer than the library is told."""
    import torch
    from genefuserust_amd import _lib
    from genefuserust_amd.hit_names import lib
    ix, _, (d1, d2), (b1, b2) = hn_texts
    hits = torch.zeros((hits_cap, 64), dtype=torch.uint8)
    hits[:len(rec)] = torch.from_numpy(rec.view(np.uint8).reshape(-1, 64).copy())
    hits = hits.cuda()
    scan_totals = torch.zeros(8, dtype=torch.int64)
    scan_totals[0] = len(rec)
    scan_totals = scan_totals.cuda()
    names = torch.full((max(names_cap + guard, 1),), FILL, dtype=torch.uint8, device="cuda")
    off = torch.full((hits_cap + 1,), -7, dtype=torch.int64, device="cuda")
    tot = torch.zeros(4, dtype=torch.int64, device="cuda")
    L = lib()
    ws_bytes = int(L.gf_hn_workspace_bytes(hits_cap))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    rc_ = L.gf_hn_names_device(ix._handle(), hits.data_ptr(), scan_totals.data_ptr(), hits_cap, HN_BASE, d1.data_ptr(),
                               d1.numel(), b1.nl_pos.data_ptr(), b1.n_newlines, d2.data_ptr(), d2.numel(),
                               b2.nl_pos.data_ptr(), b2.n_newlines, ws.data_ptr(), ws_bytes, names.data_ptr(), names_cap,
                               off.data_ptr(), tot.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc_ == _lib.GF_OK
    torch.cuda.synchronize()
    return names.cpu().numpy(), off.cpu().numpy(), [int(x) for x in tot.cpu()]


def _hn_want(hn_texts, ids, src):
    lines = hn_texts[1]
    return [lines[1 if s == 2 else 0][i] if 0 <= i < HN_RECORDS else b"" for i, s in zip(ids.tolist(), src.tolist())]


HN_FULL = HN_GRID_RECORDS + BLOCK + 1   # one block and one record more than an iteration of the lengths' grid covers


@pytest.mark.gpu
@pytest.mark.parametrize("count,hits_cap", [(SCAN_THREADS + 1, None), (2 * SCAN_THREADS + 1, None),
                                            (2 * SCAN_THREADS + 2, None), (3 * SCAN_THREADS + 1, None),
                                            (70_000, HN_FULL), (HN_FULL, HN_FULL)])
def test_hit_names_past_one_record_per_scan_thread(hn_texts, count, hits_cap):
    """per = 2, 3, 3, 4 (the last run of one, three, one, one records), and two runs through the capped grids: 70 000
    records in a buffer of HN_FULL (the grids are sized by the capacity, the runs by the number of records, which is on
    the device: per = 69, and gf_hn_k_copy strides nine times), and HN_FULL records: only a full buffer takes
    gf_hn_k_lengths' stride loop into its second iteration, with runs of HN_FULL / SCAN_THREADS + 1 records, a shorter
    last one and threads without a run."""
    hits_cap = count if hits_cap is None else hits_cap
    rec, ids, src, missing = _hn_records(count, seed=count)
    want = _hn_want(hn_texts, ids, src)
    lens = np.array([len(x) for x in want])
    need = int(lens.sum())
    names, off, tot = _hn_call(hn_texts, rec, hits_cap, need, guard=256)
    assert tot == [count, need, 0, missing] and missing >= 2
    assert (off[:count + 1] == np.concatenate([[0], np.cumsum(lens)])).all()
    assert (off[count + 1:] == -7).all()
    assert names[:need].tobytes() == b"".join(want)
    assert (names[need:] == FILL).all()
    if count == HN_FULL:
        n, per, busy, last = scan_shape(count)
        assert per == HN_FULL // SCAN_THREADS + 1 and busy < SCAN_THREADS and last < per and count > HN_GRID_RECORDS


@pytest.mark.gpu
def test_hit_names_capacity_one_byte_short_at_four_records_per_thread(hn_texts):
    count = 3 * SCAN_THREADS + 1
    rec, ids, src, missing = _hn_records(count, seed=count)
    rec["pair_id"][-1], rec["source"][-1] = HN_BASE + 200, 1          # (the last record has a name: it is the one cut)
    ids[-1], src[-1] = 200, 1
    want = _hn_want(hn_texts, ids, src)
    lens = np.array([len(x) for x in want])
    need = int(lens.sum())
    assert lens[-1] == (200 * 7 + 5) % 201 > 64
    names, off, tot = _hn_call(hn_texts, rec, count, need - 1, guard=4096)
    assert tot == [count, need, 1, missing]                            # the overflow bit, the bytes it takes
    assert (off == np.concatenate([[0], np.cumsum(lens)])).all()       # the offsets are the true ones
    fits = need - int(lens[-1])
    assert names[:fits].tobytes() == b"".join(want[:-1])               # every name that fits, in its place
    assert (names[fits:] == FILL).all()                                # the last one not started, nothing behind it


# ---- 5. reference cut: gf_rc_index_device + gf_rc_gather_device --------------------------------------------------------

KEEP_LUT = np.zeros(256, dtype=bool)
KEEP_LUT[list(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz-*")] = True
UPPER_LUT = np.arange(256, dtype=np.uint8)
UPPER_LUT[ord("a"):ord("z") + 1] -= 0x20


def fast_index(text: bytes):
    """``model_index`` of tests/test_ref_cut_plan.py in numpy (that byte loop is the yardstick; this is held to it)."""
    from genefuserust_amd.ref_cut import ChunkRecords
    a = np.frombuffer(text, dtype=np.uint8)
    rank = np.concatenate([[0], np.cumsum(KEEP_LUT[a])]).astype(np.int64)
    gt = np.flatnonzero(a == ord(">")).astype(np.int64)
    delim = np.flatnonzero((a == ord("\n")) | (a == ord(" "))).astype(np.int64)
    end = np.concatenate([gt[1:], [len(text)]]).astype(np.int64)[:gt.size]
    j = np.searchsorted(delim, gt + 1, side="left")
    cand = np.concatenate([delim, [len(text)]])[j] if gt.size else gt
    name_end = np.where(cand < end, cand, -1).astype(np.int64)
    stop = np.where(name_end >= 0, name_end, end)
    seq_rank = rank[np.where(name_end >= 0, name_end + 1, end)]
    names = [text[g + 1:s] for g, s in zip(gt.tolist(), stop.tolist())]
    unfinished = int(gt[-1]) if gt.size and name_end[-1] < 0 else -1
    return ChunkRecords(int(gt.size), int(rank[-1]), unfinished, gt, rank[gt], name_end, seq_rank, names), rank


def fast_gather(text: bytes, rec, n_records: int, rows, out_bytes: int, carried_kept: int = 0, fill: int = 0) -> bytes:
    """``model_gather`` in numpy."""
    a = np.frombuffer(text, dtype=np.uint8)
    out = np.full(out_bytes, fill, dtype=np.uint8)
    kp = np.flatnonzero(KEEP_LUT[a])
    r = np.searchsorted(rec.gt_pos, kp, side="right")
    known = r <= n_records
    kp, r = kp[known], r[known]
    seq_rank = rec.seq_rank if rec.seq_rank.size else np.zeros(1, dtype=np.int64)
    base = np.where(r == 0, -carried_kept, seq_rank[np.maximum(r, 1) - 1])
    pos = np.arange(kp.size) - base
    first = np.searchsorted(r, np.arange(n_records + 2), side="left")   # (r ascends: the kept bytes of record k)
    for k, s, e, off in rows:
        if not 0 <= k <= n_records:
            continue
        lo, hi = first[k], first[k + 1]
        sel = np.flatnonzero((pos[lo:hi] >= s) & (pos[lo:hi] < e)) + lo
        o = off + pos[sel] - s
        ok = (o >= 0) & (o < out_bytes)
        out[o[ok]] = UPPER_LUT[a[kp[sel[ok]]]]
    return out.tobytes()


def _interval_case(head: int):
    """The text and the rows of test_gather_intervals_across_tiles_and_inside_one_piece (tests/test_ref_cut_abi.py)."""
    from tests.test_ref_cut_abi import _locate
    from tests.test_ref_cut_plan import KEEP, model_index
    T = rc_tile()
    rng = np.random.default_rng(77)
    text = b">short\nACGT\n>long one\n" + b"".join(bytes(rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), 60)) + b"\n"
                                                    for _ in range(4 * T // 61))
    rec = model_index(text)
    first = next(p for p in range(T // 2 - head, len(text)) if text[p] in KEEP)
    last = next(p for p in range(3 * T - 1 - head, 0, -1) if text[p] in KEEP)
    (r0, s), (r1, e) = _locate(rec, text, first), _locate(rec, text, last)
    rows, off = [(1, 1, 3, 0)], 2
    for k in range(16):
        r, a = _locate(rec, text, 3 * T + 61 * k + k + 1 - head)
        for lo, hi in ((a, a + 3), (a + 5, a + 9)):
            rows.append((r, lo, hi, off))
            off += hi - lo
    return text, [[(2, s, e + 1, 0)], rows, []]


def _same_records(got, want):
    assert (got.n, got.kept, got.unfinished) == (want.n, want.kept, want.unfinished)
    return [f for f in ("gt_pos", "gt_rank", "name_end", "seq_rank")
            if getattr(got, f).tolist() != getattr(want, f).tolist()] + (["names"] if got.names != want.names else [])


def test_fast_reference_cut_model_equals_the_byte_loops():
    from tests.test_ref_cut_abi import CASES, _case, _whole_records
    from tests.test_ref_cut_plan import model_gather, model_index
    for name in CASES:
        for head in (0, 5, 15):
            text = _case(name, head)
            want = model_index(text)
            got, _ = fast_index(text)
            assert _same_records(got, want) == [], (name, head)
            rows = _whole_records(want, want.kept, carried=1234)
            total = max((r[3] + r[2] - r[1] for r in rows), default=0) + 8
            assert fast_gather(text, got, got.n, rows, total, 1234, FILL) == \
                model_gather(text, want, want.n, rows, total, 1234, FILL), (name, head)
            if want.unfinished >= 0:   # the text cut off in front of an unfinished header
                cut = want._replace(gt_rank=want.gt_rank[:-1], seq_rank=want.seq_rank[:-1])
                rows = _whole_records(cut, int(want.gt_rank[-1]))
                total = max((r[3] + r[2] - r[1] for r in rows), default=0) + 8
                nb = want.unfinished
                assert fast_gather(text[:nb], got, got.n - 1, rows, total, 0, FILL) == \
                    model_gather(text[:nb], want, want.n - 1, rows, total, 0, FILL), (name, head)
    for head in (0, 9):
        text, row_sets = _interval_case(head)
        want = model_index(text)
        got, _ = fast_index(text)
        assert _same_records(got, want) == []
        for rows in row_sets:
            total = max((r[3] + r[2] - r[1] for r in rows), default=0) + 8
            assert fast_gather(text, got, got.n, rows, total, 0, FILL) == model_gather(text, want, want.n, rows, total, 0, FILL)


RC_RUN_BOUNDARY = SCAN_THREADS // 2 - 1     # the thread whose run starts with a '>' on either side of it
RC_SHORT_RECORDS = 2 * SCAN_THREADS + 40


def rc_big_text(head: int) -> bytes:
    """(SCAN_THREADS + 2) tiles and 517 bytes: bytes in front of the first '>'; RC_SHORT_RECORDS short records with
    names of 0 .. 150 bytes, some empty, some with a '>' inside the header; long records in lines of 60 letters with
    lower case, '-', '*' and digits; short records on both sides of tile SCAN_THREADS and across the run boundaries of
    threads 1, 2 and WAVE - 1; a '>' on the last byte of tile 2 k - 1 and one on the first byte of tile 2 k for
    k = RC_RUN_BOUNDARY; the last header unfinished."""
    T = rc_tile()
    size = (SCAN_THREADS + 2) * T + 517
    rng = np.random.default_rng(41)
    out = bytearray(b"ACGTacgtNN-*\nGGCC 12\n")
    for k in range(RC_SHORT_RECORDS):
        ln = k % 151
        name = (b"n%d_" % k + b"x" * ln)[:ln]
        if k % 17 == 5:
            name = name[:ln // 2] + b">" + name[ln // 2:]
        out += b">" + name + (b" d\n", b"\n", b"\td e\n")[k % 3] + b"ACGTacgt-*N7"[:1 + k % 12] + b"\n"
    alphabet = np.frombuffer(b"ACGTACGTACGTacgtnN-*7", dtype=np.uint8)
    tail = b">the_last_header_is_not_finished"
    nlines = size // 61 + 1
    body = np.concatenate([rng.choice(alphabet, (nlines, 60)), np.full((nlines, 1), ord("\n"), dtype=np.uint8)], axis=1)
    for k in range(0, nlines, 3000):
        out += b">long%d of many lines\n" % k + body[k:k + 3000].tobytes()
    out = out[:size]
    at = lambda grid: grid - head   # the text byte at a place on the grid of addresses
    side = b"\n>s%d d\nACGTAC\n>t%d\nGG-*cc\n"
    for j, thread in enumerate((1, 2, WAVE - 1)):
        snip = side % (j, j)
        out[at(2 * thread * T - 12):at(2 * thread * T - 12) + len(snip)] = snip
    snip = b"\n>left_a d\nACGTAC\n>left_b\nGG-*cc\nTT\n"
    out[at(SCAN_THREADS * T) - len(snip) - 3:at(SCAN_THREADS * T) - 3] = snip
    snip = b"\n>right_a\nTTTTGG\n>right_b x\nacgt\nAC\n"
    out[at(SCAN_THREADS * T) + 5:at(SCAN_THREADS * T) + 5 + len(snip)] = snip
    out[at(2 * RC_RUN_BOUNDARY * T - 1)] = ord(">")
    out[at(2 * RC_RUN_BOUNDARY * T)] = ord(">")
    out[size - len(tail):] = tail
    return bytes(out)


def rc_gather_rows(text: bytes, rec, rank, head: int, carried: int):
    """About 40 rows, sorted by record and start: the bytes in front of the first '>' as a record carried in, whole
    short records at the front and on both sides of tile SCAN_THREADS, intervals from tile 2 k - 1 into tile 2 k, and
    one of three tiles that ends in the last tile."""
    T = rc_tile()
    a = np.frombuffer(text, dtype=np.uint8)
    kept_pos = np.flatnonzero(KEEP_LUT[a])

    def locate(p):   # (record ordinal, contig position) of the first kept byte at or behind text byte p
        p = int(kept_pos[np.searchsorted(kept_pos, p)])
        r = int(np.searchsorted(rec.gt_pos, p, side="right"))
        return r, int(rank[p]) - (int(rec.seq_rank[r - 1]) if r else -carried)

    def whole(r):    # every sequence byte of record r >= 1
        end = int(rec.gt_rank[r]) if r < rec.n else rec.kept
        return (r, 0, end - int(rec.seq_rank[r - 1]))

    wanted = [(0, carried, carried + int(rec.gt_rank[0]))]
    wanted += [whole(r) for r in range(1, 31)]
    mid = int(np.searchsorted(rec.gt_pos, SCAN_THREADS * T - head))   # records that start in front of tile SCAN_THREADS
    wanted += [whole(r) for r in (mid - 1, mid, mid + 1)]   # (the three-tile interval below is of record mid + 2)
    straddling = 0
    for thread in (WAVE, WAVE + 1, RC_RUN_BOUNDARY - 2, RC_RUN_BOUNDARY - 1):
        (r0, s), (r1, e) = locate(2 * thread * T - 100 - head), locate(2 * thread * T + 100 - head)
        if r0 == r1 and 0 <= s < e:
            wanted.append((r0, s, e))
            straddling += 1
    ntiles = -(-(head + len(text)) // T)
    (r0, s), (r1, e) = locate((ntiles - 3) * T + 200 - head), locate(rec.unfinished - 70)
    assert r0 == r1 and e - s > 2 * T * 50 // 61 and straddling >= 3
    wanted.append((r0, s, e))
    wanted = sorted(w for w in set(wanted) if w[2] > w[1])
    rows, off = [], 0
    for r, s, e in wanted:
        rows.append((r, s, e, off))
        off += e - s
    return rows, off


def test_reference_cut_text_crosses_the_thresholds():
    from genefuserust_amd.ref_cut import lib
    T = rc_tile()
    for head in (0, 7):
        text = rc_big_text(head)
        assert len(text) == (SCAN_THREADS + 2) * T + 517
        ntiles, per, busy, last = scan_shape(int(lib().gf_rc_tiles(len(text))))
        assert ntiles == -(-(head + len(text)) // T) > SCAN_THREADS and per == 2 and last < per and busy < SCAN_THREADS
        rec, rank = fast_index(text)
        n, per, busy, last = scan_shape(rec.n)
        assert rec.n > 2 * SCAN_THREADS and per == 3 and busy < SCAN_THREADS
        assert rec.unfinished == len(text) - len(b">the_last_header_is_not_finished")
        g = rec.gt_pos + head
        k = 2 * RC_RUN_BOUNDARY
        assert k * T - 1 in g and k * T in g and b"" in rec.names and max(len(x) for x in rec.names) >= 150
        assert ((g // T) >= SCAN_THREADS).sum() >= 3 and rec.gt_rank[0] > 0
        rows, total = rc_gather_rows(text, rec, rank, head, 1234)
        assert 35 <= len(rows) <= 45
        assert all((a[0], a[2]) <= (b[0], b[1]) for a, b in zip(rows, rows[1:]))   # disjoint, sorted


@pytest.mark.gpu
@pytest.mark.parametrize("head", [0, 7])
def test_reference_cut_past_one_tile_per_scan_thread(gpu_device, head):
    import torch
    from genefuserust_amd.ref_cut import lib, ref_gather_device, ref_index_device
    from tests.test_ref_cut_abi import _device
    T = rc_tile()
    text = rc_big_text(head)
    want, rank = fast_index(text)
    d = _device(text, head)
    need = sum(len(x) for x in want.names)
    ix = ref_index_device(d, want.n, need)
    got = ix.download()
    bad = _same_records(got, want)
    ntiles = -(-(head + len(text)) // T)
    want_tiles = rank[np.maximum(np.arange(ntiles) * T - head, 0)].tolist() + [int(rank[-1])]
    if ix.tile_kept[:ntiles + 1].cpu().tolist() != want_tiles:
        bad.append("tile_kept")
    assert bad == []
    rows, total = rc_gather_rows(text, want, rank, head, 1234)
    out = torch.full((total + 8,), FILL, dtype=torch.uint8, device="cuda")
    ref_gather_device(d, ix, want.n, rows, total + 8, 1234, out=out)
    res = out.cpu().numpy().tobytes()
    assert res == fast_gather(text, want, want.n, rows, total + 8, 1234, FILL)
    assert FILL not in res[:total] and res[total:] == bytes([FILL]) * 8
    # cap_records one short: the overflow bit, the first cap entries, the sentinels behind them
    cap = want.n - 1
    L = lib()
    i64 = lambda n, v=-7: torch.full((n,), v, dtype=torch.int64, device="cuda")
    arrays = [i64(cap + 4) for _ in range(4)]
    name_off, names, totals = i64(cap + 5), torch.full((need + 64,), FILL, dtype=torch.uint8, device="cuda"), i64(8)
    ws = torch.empty(int(L.gf_rc_workspace_bytes(len(text))), dtype=torch.uint8, device="cuda")
    tile_kept = i64(int(L.gf_rc_tiles(len(text))) + 1)
    assert L.gf_rc_index_device(d.data_ptr(), len(text), cap, ws.data_ptr(), ws.numel(), *(a.data_ptr() for a in arrays),
                                name_off.data_ptr(), names.data_ptr(), need, tile_kept.data_ptr(), totals.data_ptr(),
                                None) == 0
    torch.cuda.synchronize()
    tot = totals.cpu().tolist()
    assert tot[0] == want.n and tot[1] == want.kept and tot[2] & 1
    for a, f in zip(arrays, ("gt_pos", "gt_rank", "name_end", "seq_rank")):
        if f in ("gt_pos", "gt_rank"):
            assert a[:cap].cpu().tolist() == getattr(want, f)[:cap].tolist(), f
        assert a[cap:].cpu().tolist() == [-7] * 4, f
    assert name_off[cap + 1:].cpu().tolist() == [-7] * 4
    assert tile_kept[:ntiles + 1].cpu().tolist() == want_tiles
