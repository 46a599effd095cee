"""Seed+verify at its edges, read by read against the oracle (r05).

r05 took instructions out of code that runs for every read — the verification's clean windows are chained from the
last word down and gathered by a dot product, and the 10-word form cuts a read's packed words out of the LDS tile once,
for the seeds, the verification, the queue record and the list entry alike — so the cases put tiles, waves, blocks, the
wave's queue and the staging loop at their boundaries, and the reads of tests/gate_reads.py, which sit next to
map_read's gates, among ordinary ones: a verified window too many or too few, or a queue record with a wrong word, ends
(or keeps) one of them.

Every case goes through map_reads_device, map_reads_packed_device and — where its reads all have one length, the only
batches that route takes — map_reads_fixed_device; counts and matches are compared with OracleIndexer.map_reads_packed
on every read.  Index: IDX-T at scale 0.05 with 10 % repeats, as tests/test_gate_reads.py; twice: with the default
filter (16 bits per key here: background reads end in round 0) and with one of 1.75 bits per key, the least that stays
L2-resident and so keeps the queue in use (nearly every look-up answers "present": records outlive round 0, are queued
again for round 1 and leave for the list).

A wave meets more than one tile only beyond 256 reads per block — a quarter of a million reads at the default launch
geometry — so the cases about what a wave's queue carries from tile to tile run 131 072 reads with GF_NBLK_MULT=1 (one
block per CU: 512 reads a block on the MI355X's 256 CUs, two tiles a wave).
"""
import functools
import os

import numpy as np
import pytest

from tests.gate_reads import gate_reads

L0 = 150
_EXPECT = {}


@functools.lru_cache(maxsize=None)
def _genes():
    from genefuserust_amd import synth
    return synth.make_geneset("IDX-T", scale=0.05, repeat_frac=0.1)


@functools.lru_cache(maxsize=None)
def _pool(kind, read_len, n, seed):
    """n reads of one kind ("bg" background, "on" single gene, "panel" the benchmark's mix) as uint8[n, read_len]."""
    from genefuserust_amd import synth
    synth.MIXES["SVB_BG"] = (1.0, 0.0, 0.0)
    synth.MIXES["SVB_ON"] = (0.0, 1.0, 0.0)
    mix = {"bg": "SVB_BG", "on": "SVB_ON", "panel": "PANEL"}[kind]
    if read_len < 60:   # (make_reads places a junction's break 30 bases from either end: shorter reads are cut from longer)
        return _pool(kind, 100, n, seed)[:, :read_len].copy()
    rb = synth.make_reads(_genes(), n, read_len=read_len, mix=mix, seed=seed)
    return rb.bases.numpy().reshape(n, read_len).copy()


def _fixed(rows):
    n, L = rows.shape
    return np.ascontiguousarray(rows).reshape(-1), np.arange(n + 1, dtype=np.int64) * L


def _panel(n, read_len=L0, bg_share=None, seed=1):
    """n reads of one length: the benchmark's mix, or `bg_share` of them background (drawn per read, seeded)."""
    if bg_share is None:
        return _fixed(_pool("panel", read_len, n, 100 + seed))
    rows = _pool("on", read_len, n, 200 + seed).copy()
    is_bg = np.random.default_rng(300 + seed).random(n) < bg_share
    rows[is_bg] = _pool("bg", read_len, n, 400 + seed)[is_bg]
    return _fixed(rows)


@functools.lru_cache(maxsize=None)
def _wave_batch():
    """131 072 reads, 512 a block with GF_NBLK_MULT=1 on 256 CUs: wave 0 of block b maps reads 512b .. 512b+63 and
    512b+256 .. 512b+319.  On-target reads but for the background reads placed so that a wave's queue holds, after its
    two tiles: 63 (one partial pass at the end), 64 (one full pass after the second tile), 65 (a full pass, then one of
    a single record); a block of background only (a full pass per tile and wave); 50 + 50 (more than the queue's 96
    places: a pass runs before the second tile's records go in); then 40 blocks at 75 % background (the same, at
    random), and the benchmark's mix for the rest."""
    n = 131072
    rows = _pool("on", L0, n, 11).copy()
    bg = _pool("bg", L0, n, 12)
    take = np.zeros(n, dtype=bool)
    for b, (t1, t2) in enumerate([(40, 23), (40, 24), (40, 25)]):
        take[512 * b:512 * b + t1] = True
        take[512 * b + 256:512 * b + 256 + t2] = True
    take[512 * 3:512 * 4] = True
    take[512 * 4:512 * 4 + 50] = True
    take[512 * 4 + 256:512 * 4 + 256 + 50] = True
    rng = np.random.default_rng(13)
    take[512 * 5:512 * 45] = rng.random(512 * 40) < 0.75
    take[512 * 45:] = rng.random(n - 512 * 45) < 0.40
    rows[take] = bg[take]
    return _fixed(rows)


@functools.lru_cache(maxsize=None)
def _gate_batch(exact_len):
    """The gate reads of up to 160 bases (exact_len: of exactly that many) shuffled among three times as many reads of
    the benchmark's mix."""
    from genefuserust_amd import synth
    gate = [r for _, r in gate_reads(_genes().seqs, seed=2024, n=4000)
            if (len(r) == exact_len if exact_len else len(r) <= 160)]
    assert len(gate) > (300 if exact_len else 1000)
    fill_len = exact_len or L0
    fill = _pool("panel", fill_len, 3 * len(gate), 21)
    reads = gate + [row.tobytes() for row in fill]
    order = np.random.default_rng(22).permutation(len(reads))
    return synth.ragged_batch([reads[k] for k in order])


@functools.lru_cache(maxsize=None)
def _mixed_lengths():
    from genefuserust_amd import synth
    reads = []
    for L in LENGTHS:
        reads += [row.tobytes() for row in _pool("panel", L, 100, 31)]
    order = np.random.default_rng(32).permutation(len(reads))
    return synth.ragged_batch([reads[k] for k in order])


SIZES = (1, 63, 64, 65, 255, 256, 257)
LENGTHS = (54, 55, 100, 149, 150, 151, 160)

# name -> (batch builder, max_read_len, environment of the call)
CASES = {}
for _n in SIZES:
    CASES["n%d" % _n] = (functools.partial(_panel, _n), 160, {})
CASES["background_6145"] = (functools.partial(_panel, 64 * 96 + 1, L0, 1.0, 2), 160, {})
for _k in (63, 64, 65):   # ... background reads among on-target ones, at the default geometry: within one block's 256 reads
    def _some_bg(k=_k):
        rows = _pool("on", L0, 256, 40 + k).copy()
        at = np.random.default_rng(k).permutation(128)[:k]   # (the block's first two waves: up to 64 each)
        rows[at] = _pool("bg", L0, 256, 50 + k)[at]
        return _fixed(rows)
    CASES["background_%d_of_256" % _k] = (_some_bg, 160, {})
CASES["wave_two_tiles"] = (_wave_batch, 160, {"GF_NBLK_MULT": "1"})
for _L in LENGTHS:
    CASES["len%d" % _L] = (functools.partial(_panel, 257, _L), 160, {})
CASES["mixed_lengths"] = (_mixed_lengths, 160, {})
CASES["class256_len200"] = (functools.partial(_panel, 257, 200), 256, {})
CASES["class320_len300"] = (functools.partial(_panel, 257, 300), 320, {})
CASES["gate_reads"] = (functools.partial(_gate_batch, 0), 160, {})
CASES["gate_reads_150"] = (functools.partial(_gate_batch, 150), 160, {})

TIGHT_CASES = ("n257", "background_6145", "background_65_of_256", "wave_two_tiles", "len160", "mixed_lengths", "gate_reads",
               "gate_reads_150")


def _expected(oracle, name, bases, offsets):
    if name not in _EXPECT:
        ox = oracle.OracleIndexer(_genes().seqs)
        _EXPECT[name] = ox.map_reads_packed(bases, offsets, threads=8)
        ox.close()
    return _EXPECT[name]


def _make_index(tight):
    """tight: the filter at 1.75 bits per site (gfmatch.hip make_filter: the least it keeps L2-resident)."""
    from genefuserust_amd import Indexer
    genes = _genes()
    old = os.environ.get("GF_BLOOM_KIB")
    try:
        if tight:
            ix = Indexer.from_gene_slices(genes.seqs, genes.reversed_flags)
            ix.make_index()
            sites = ix.info()["n_sites"]
            ix.close()
            # the build wants 7 / 128 words per site at least, or the filter is no longer asked from seed+verify: that, and
            # a KiB to spare, as the cap
            os.environ["GF_BLOOM_KIB"] = str((sites * 7 // 128 * 4 + 1023) // 1024 + 1)
        ix = Indexer.from_gene_slices(genes.seqs, genes.reversed_flags)
        ix.make_index()
    finally:
        if old is None:
            os.environ.pop("GF_BLOOM_KIB", None)
        else:
            os.environ["GF_BLOOM_KIB"] = old
    return ix


@pytest.fixture(scope="module")
def indexes(gpu_device):
    made = {}

    def get(tight):
        if tight not in made:
            made[tight] = _make_index(tight)
        return made[tight]

    yield get
    for ix in made.values():
        ix.close()


def _host(counts, matches, n):
    import torch
    from genefuserust_amd import _lib
    torch.cuda.synchronize()
    c = counts.cpu().numpy().astype(np.int32)[:n]
    m = matches.cpu().numpy().view(_lib.SEQMATCH_DTYPE).reshape(-1, 2)[:n]
    return c, m


def _differences(label, got, want):
    (counts, matches), (ocounts, omatches) = got, want
    assert counts.shape == ocounts.shape, label
    bad = counts != ocounts
    bad |= (ocounts > 0) & (matches[:, 0] != omatches[:, 0])
    bad |= (ocounts == 2) & (matches[:, 1] != omatches[:, 1])
    if not bad.any():
        return []
    rows = np.nonzero(bad)[0]
    return ["%s: %d of %d reads differ from the oracle, first %s (got count %s, want %s)" % (
        label, rows.size, counts.size, rows[:8].tolist(), counts[rows[:8]].tolist(), ocounts[rows[:8]].tolist())]


def _on_device(bases, shift):
    """`bases` in device memory, its first byte `shift` bytes past a 256-byte boundary."""
    import torch
    buf = torch.zeros(bases.size + shift + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    d = buf[shift:shift + bases.size]
    d.copy_(torch.from_numpy(bases))
    return d


def _run_routes(ix, label, bases, offsets, cap, want, shift=0):
    import torch
    n = offsets.size - 1
    problems = []
    d_b, d_o = _on_device(bases, shift), torch.from_numpy(offsets).cuda()
    got = _host(*ix.map_reads_device(d_b, d_o, cap), n)
    problems += _differences("%s, map_reads_device" % label, got, want)
    pk, iv = ix.pack_bases_device(d_b)
    got = _host(*ix.map_reads_packed_device(pk, iv, d_o, cap), n)
    problems += _differences("%s, map_reads_packed_device" % label, got, want)
    lens = np.diff(offsets)
    if n > 0 and (lens == lens[0]).all():
        got = _host(*ix.map_reads_fixed_device(d_b, int(lens[0])), n)
        problems += _differences("%s, map_reads_fixed_device" % label, got, want)
    return problems


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_case_equals_oracle(indexes, oracle, name):
    build, cap, env = CASES[name]
    bases, offsets = build()
    want = _expected(oracle, name, bases, offsets)
    problems = _with_env(env, lambda: _run_routes(indexes(False), name, bases, offsets, cap, want))
    if problems:
        pytest.fail("\n".join(problems))


@pytest.mark.gpu
@pytest.mark.parametrize("name", TIGHT_CASES)
def test_case_equals_oracle_with_a_filter_that_passes_most(indexes, oracle, name):
    build, cap, env = CASES[name]
    bases, offsets = build()
    want = _expected(oracle, name, bases, offsets)
    problems = _with_env(env, lambda: _run_routes(indexes(True), name + ", tight filter", bases, offsets, cap, want))
    if problems:
        pytest.fail("\n".join(problems))


@pytest.mark.gpu
@pytest.mark.parametrize("read_len", [150, 160])
def test_bases_off_a_16_byte_boundary(indexes, oracle, read_len):
    """`bases` 1 to 15 bytes past a 16-byte boundary: a tile then starts `mis` bytes into its first chunk, and 64 reads of
    160 bases — 640 chunks, ten whole staging iterations at shift 0 — spill one chunk into the eleventh."""
    bases, offsets = _panel(257, read_len, seed=7)
    want = _expected(oracle, "shift%d" % read_len, bases, offsets)
    problems = []
    for shift in range(1, 16):
        problems += _run_routes(indexes(False), "%d bases, shift %d" % (read_len, shift), bases, offsets, 160, want, shift)
    if problems:
        pytest.fail("\n".join(problems))


def test_cases_cover_what_the_issue_lists():
    """(CPU) the batch sizes, lengths and placements exist as cases; the two-tile batch places what its docstring says."""
    assert all("n%d" % n in CASES for n in SIZES) and all("len%d" % L in CASES for L in LENGTHS)
    assert CASES["background_6145"][0]()[1].size - 1 == 64 * 96 + 1
    assert set(TIGHT_CASES) <= set(CASES)
