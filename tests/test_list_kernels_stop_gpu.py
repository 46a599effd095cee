"""The list kernels where they stop early, read by read against the oracle (r07).

gf_k_probe_buckets leaves its probe loop once a read that has its diagonal can no longer die (v1 + h >= 20 and
v2 + h >= 10; never while it still wants its diagonal, because finding K takes votes out of h).  Handing a read to the
exact kernel is always exact; what can go wrong is a mask or a counter — a window asked twice or never, a word cut at
the wrong place, `left` off by one — a read declared dead one vote early, or the early exit taken while the diagonal is
still wanted.  Such errors show only on reads next to a gate, so the cases are:

  gate reads        tests/gate_reads.py (seed 2024, n = 4000) by length class: max_read_len 160, 256 and 320 pick the
                    10-, 16- and 20-word instantiations
  junction reads    a minor part of 32 to 75 bases: 9 standing windows (dead on v2 + h + left < 10 without a probe) up to
                    30 (the early exit after one, two or three rounds); 150, 250 and 300 bases; and minor parts of 18 to
                    30 bases at one end or at both, whose standing windows lie in one word or eight words apart
  mismatch places   on-target reads with substitutions that open windows in the first word only, the last word only, the
                    first and the last, every other word, every word (a substitution in mid-word every 32 bases), and
                    spread over the read
  no diagonal       on-target reads with a substitution inside each of bases 0-15, 32-47, 64-79 and 96-111 (seed+verify
                    finds no diagonal: gf_k_probe_buckets has to), half of them cut from a duplicated stretch, where h
                    has grown before K is found
  chunks            131 072 reads with GF_NBLK_MULT=1 (512 a block), three quarters on-target reads with two substitution
                    clusters (more than 256 entries a block: a second chunk in gf_k_probe_filter), and the reads of every
                    family above as reads 192 to 320 of a block of its own.  Where a read's entry lands in its block's
                    list is not fixed — seed+verify deals a block's reads to its waves by tile and the waves append in
                    no fixed order — so the family reads are spread around the 256th entry instead of being placed on it

each shuffled among three times as many reads of the benchmark's mix, on the index of tests/test_seedverify_budget_gpu.py
(IDX-T at scale 0.05, 10 % repeats) with the default filter and with one of 1.75 bits per site (look-ups mostly pass),
through map_reads_device, map_reads_packed_device and, where the lengths allow, map_reads_fixed_device; counts and
matches of EVERY read are compared with OracleIndexer.map_reads_packed.

The CPU test states, on the Python model's trace, that the batches do hold the reads the kernels decide by one vote.
"""
import functools

import numpy as np
import pytest

from oracle import indexer_model as M
from tests import test_seedverify_budget_gpu as SV
from tests.gate_reads import _dupe_stretches, _junction, _part, _substitute, gate_reads
from tests.helpers import rc

FLOOR = 20
CLASS_FILL = {160: 150, 256: 250, 320: 300}   # max_read_len -> length of the filler reads
CHUNK_SPAN = (192, 320)                       # the chunk batch: a family's reads of its block, first and last


def _genes():
    return SV._genes()


def _one_gene(rng, genes, n):
    return bytearray(_part(rng, genes, n))


@functools.lru_cache(maxsize=None)
def _usable_genes():
    return tuple(g for g in _genes().seqs if g is not None and len(g) >= 640)


@functools.lru_cache(maxsize=None)
def _families():
    """name -> list of reads (bytes).  Seeded; the same on every call."""
    genes = _usable_genes()
    rng = np.random.default_rng(707)
    fam = {}

    def flip(read):
        read = bytes(read)
        return rc(read) if rng.random() < 0.5 else read

    for L in (150, 250, 300):
        out = []
        for m in [32, 33] * 30 + list(range(34, 76)) * (8 if L == 150 else 3):
            out.append(flip(_junction(rng, genes, L, m if rng.random() < 0.5 else L - m)))
        fam["junction_%d" % L] = out
    out = []
    for k in range(240):   # short minor parts: their standing windows lie in one word, or at both ends of the read
        m = int(rng.integers(18, 31))
        if k % 2 == 0:
            out.append(flip(_junction(rng, genes, 150, m)))
        else:
            m2 = int(rng.integers(18, 31))
            out.append(flip(_part(rng, genes, m) + _part(rng, genes, 150 - m - m2) + _part(rng, genes, m2)))
    fam["short_minor"] = out

    def with_subs(L, places):
        read = _one_gene(rng, genes, L)
        for p in places:
            _substitute(rng, read, p)
        return bytes(read)     # (not flipped: the places are places of the read as mapped)

    for L in (150, 250, 300):
        out = []
        for _ in range(60):
            out.append(with_subs(L, rng.integers(0, 15, size=int(rng.integers(2, 4)))))                 # first word only
            out.append(with_subs(L, L - 1 - rng.integers(0, 7, size=int(rng.integers(2, 4)))))          # last word only
            out.append(with_subs(L, list(rng.integers(0, 15, size=2)) + list(L - 1 - rng.integers(0, 7, size=2))))
            out.append(with_subs(L, [p for p in range(15, L - 8, 32)][:5]))                             # every other word
            out.append(with_subs(L, np.sort(rng.integers(0, L, size=3))))                               # spread
        fam["placement_%d" % L] = out
    # every word: a substitution at base b opens the windows that start at b - 15 .. b, so one in mid-word, every 32
    # bases from base 20 on, opens windows in two adjacent words each and in every word of the read together (150 bases:
    # 20, 52, 84, 116, 148 -> words 0-1, 2-3, 4-5, 6-7, 8); half of the windows still vote, so the diagonal stands.
    # (A generator of its own: the families above stay what they were.)
    rng_w = np.random.default_rng(708)
    for L in (150, 250, 300):
        for _ in range(60):
            read = _one_gene(rng_w, genes, L)
            for p in range(20, L, 32):
                _substitute(rng_w, read, p)
            fam["placement_%d" % L].append(bytes(read))

    stretches = _dupe_stretches(genes, min_windows=150 - 15)
    assert stretches, "no duplicated stretch of 135 windows in the genes: the h -= nh reads cannot be cut"
    out = []
    for k in range(300):
        if k % 2:
            gi, a, nw = stretches[int(rng.integers(0, len(stretches)))]
            p = a + int(rng.integers(0, nw + 15 - 150 + 1))
            read = bytearray(genes[gi][p:p + 150].upper())
            if rng.random() < 0.5:
                read = bytearray(rc(bytes(read)))
        else:
            read = _one_gene(rng, genes, 150)
        for lo in (0, 32, 64, 96):
            _substitute(rng, read, lo + int(rng.integers(0, 16)))
        out.append(bytes(read))
    fam["no_diagonal"] = out
    return fam


@functools.lru_cache(maxsize=None)
def _gate_by_class():
    by = {160: [], 256: [], 320: []}
    for _, r in gate_reads(_genes().seqs, seed=2024, n=4000):
        by[160 if len(r) <= 160 else (256 if len(r) <= 256 else 320)].append(r)
    return by


def _class_of(name):
    return {"250": 256, "300": 320}.get(name.rsplit("_", 1)[-1], 160)


@functools.lru_cache(maxsize=None)
def _shuffled(name):
    """The case's reads among three times as many reads of the benchmark's mix, as (bases, offsets)."""
    from genefuserust_amd import synth
    if name.startswith("gate_"):
        cap = int(name[5:])
        reads = _gate_by_class()[cap]
    else:
        cap = _class_of(name)
        reads = _families()[name]
    fill = SV._pool("panel", CLASS_FILL[cap], 3 * len(reads), 71)
    reads = list(reads) + [row.tobytes() for row in fill]
    order = np.random.default_rng(72).permutation(len(reads))
    return synth.ragged_batch([reads[k] for k in order])


def _clustered(rng, rows):
    """Two substitution clusters (widths 1 to 5) in every row of uint8[n, L], in place."""
    n, L = rows.shape
    other = np.frombuffer(b"CATG", dtype=np.uint8)   # A->C, C->A, G->T, T->G by position in "ACGT"
    code = np.zeros(256, dtype=np.uint8)
    for k, ch in enumerate(b"ACGT"):
        code[ch] = k
    for _ in range(2):
        w = rng.integers(1, 6, size=n)
        p = rng.integers(0, L - 5, size=n)
        for q in (p, p + w - 1):
            rows[np.arange(n), q] = other[code[rows[np.arange(n), q]]]
    return rows


@functools.lru_cache(maxsize=None)
def _chunk_batch():
    """131 072 reads of 150 bases, 512 a block with GF_NBLK_MULT=1 (see the module's docstring)."""
    n = 131072
    rng = np.random.default_rng(81)
    rows = SV._pool("panel", SV.L0, n, 82).copy()
    on = _clustered(rng, SV._pool("on", SV.L0, n, 83).copy())
    take = rng.random(n) < 0.75
    take[:512 * 24] = True          # the blocks that get the family reads hold entry-making reads only
    rows[take] = on[take]
    fams = [v for k, v in sorted(_families().items()) if _class_of(k) == 160]
    fams.append([r for r in _gate_by_class()[160] if len(r) == SV.L0])
    b = 0
    for reads in fams:
        picks = [r for r in reads if len(r) == SV.L0]
        for k, at in enumerate(range(512 * b + CHUNK_SPAN[0], 512 * b + CHUNK_SPAN[1] + 1)):
            rows[at] = np.frombuffer(picks[(7 * k) % len(picks)], dtype=np.uint8)   # a block a family, around entry 256
        b += 1
    assert b <= 24
    return SV._fixed(rows)


# name -> (batch builder, max_read_len, environment of the call)
CASES = {}
for _cap in (160, 256, 320):
    CASES["gate_%d" % _cap] = (functools.partial(_shuffled, "gate_%d" % _cap), _cap, {})
for _name in ("junction_150", "junction_250", "junction_300", "short_minor", "placement_150", "placement_250",
              "placement_300", "no_diagonal"):
    CASES[_name] = (functools.partial(_shuffled, _name), _class_of(_name), {})
CASES["chunks"] = (_chunk_batch, 160, {"GF_NBLK_MULT": "1"})


@pytest.fixture(scope="module")
def indexes(gpu_device):
    made = {}

    def get(tight):
        if tight not in made:
            made[tight] = SV._make_index(tight)
        return made[tight]

    yield get
    for ix in made.values():
        ix.close()


_EXPECT = {}


def _expected(oracle, name, bases, offsets):
    if name not in _EXPECT:   # computed once, shared by the two filter builds
        ox = oracle.OracleIndexer(_genes().seqs)
        _EXPECT[name] = ox.map_reads_packed(bases, offsets, threads=8)
        ox.close()
    return _EXPECT[name]


@pytest.mark.gpu
@pytest.mark.parametrize("tight", [False, True], ids=["default_filter", "filter_passes_most"])
@pytest.mark.parametrize("name", list(CASES))
def test_case_equals_oracle(indexes, oracle, name, tight):
    build, cap, env = CASES[name]
    bases, offsets = build()
    want = _expected(oracle, name, bases, offsets)
    label = name + (", tight filter" if tight else "")
    problems = SV._with_env(env, lambda: SV._run_routes(indexes(tight), label, bases, offsets, cap, want))
    if problems:
        pytest.fail("\n".join(problems))


@functools.lru_cache(maxsize=None)
def _model():
    return M.IndexModel([s.decode() for s in _genes().seqs])


def _off_diagonal_windows(mx, read, gp1):
    """The read's stride-2 windows (by number) whose key is in the table and that do not vote for diagonal gp1."""
    out = []
    for i in range(0, len(read) - M.K + 1, 2):
        k = M.kmer_at(read, i)
        if k is None or mx.table.get(k) is None:
            continue
        if not any(M.key64(c, p - i) == gp1 for (c, p) in mx.sites(k)):
            out.append(i // 2)
    return out


def test_batches_hold_the_reads_the_list_kernels_decide_by_one_vote():
    """(CPU) floors on the reference's own trace, before any GPU sees the batches."""
    mx = _model()
    reads = [r for rs in _families().values() for r in rs] + [r for rs in _gate_by_class().values() for r in rs]
    n = {}

    def hit(name):
        n[name] = n.get(name, 0) + 1

    for read in reads:
        s = read.decode()
        t = mx.map_read_trace(s)
        c1, c2, _ = t.votes
        if not t.segments:
            if 18 <= c1 <= 21:
                hit("ends [], first %d" % c1)
            if 8 <= c2 <= 12:
                hit("ends [], second %d" % c2)
        if c1 >= 20:
            gp1 = M.key64(*t.diagonals[0])
            off = _off_diagonal_windows(mx, s, gp1)
            if len(off) in (9, 10, 11):
                hit("off-diagonal %d" % len(off))
            if off and off[0] >> 3 == off[-1] >> 3:
                hit("off-diagonal in one word")
            if off and (off[-1] >> 3) - (off[0] >> 3) >= 8:
                hit("off-diagonal eight words apart")
            # windows the verification on gp1 leaves open (no vote for gp1, in the table or not), by word of 8 windows
            starts = range(0, len(s) - M.K + 1, 2)
            open_words = {i >> 4 for i in starts
                          if not any(M.key64(c, p - i) == gp1 for (c, p) in mx.sites(M.kmer_at(s, i)))}
            if open_words == {i >> 4 for i in starts}:
                hit("open windows in every word, %d bases" % len(s))
    floors = ["ends [], first %d" % v for v in (18, 19, 20, 21)] + ["ends [], second %d" % v for v in (8, 9, 10, 11, 12)]
    floors += ["off-diagonal %d" % v for v in (9, 10, 11)] + ["off-diagonal in one word", "off-diagonal eight words apart"]
    floors += ["open windows in every word, %d bases" % L for L in (150, 250, 300)]   # (each with a diagonal of 20 votes or more)
    print(sorted(n.items()))
    short = {k: n.get(k, 0) for k in floors if n.get(k, 0) < FLOOR}
    assert not short, short


def test_cases_cover_what_the_issue_lists():
    """(CPU) every length class, every family, the chunk batch's size and its planted reads."""
    assert {c for _, c, _ in CASES.values()} == {160, 256, 320}
    fam = _families()
    assert all(len(v) >= 150 for v in fam.values())
    assert all(len(v) > 300 for v in _gate_by_class().values())
    bases, offsets = _chunk_batch()
    assert offsets.size - 1 == 131072 and CASES["chunks"][2] == {"GF_NBLK_MULT": "1"}
    row = bases.reshape(-1, SV.L0)
    names = sorted(k for k in fam if _class_of(k) == 160)
    assert "no_diagonal" in names and "placement_150" in names
    for b, name in enumerate(names):   # a block a family, its reads on either side of the block's 256th
        own = set(fam[name])
        assert all(row[512 * b + at].tobytes() in own for at in range(CHUNK_SPAN[0], CHUNK_SPAN[1] + 1)), name
    assert CHUNK_SPAN[0] < 256 < CHUNK_SPAN[1]
    # the every-word placement is in every placement family, and half of the no-diagonal reads come from a duplicated stretch
    assert all(len(fam["placement_%d" % L]) == 360 for L in (150, 250, 300))
    assert len(_dupe_stretches(_usable_genes(), min_windows=150 - 15)) > 0
