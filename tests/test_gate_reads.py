"""map_read's gates, held to the oracle on junction reads with errors (tests/gate_reads.py).

The flat pipeline ends a read with [] only when it proves that the read fails the vote gate
(DESIGN.md §4); a proof that is off by one vote shows only on a read next to a gate.  The CPU
tests state that the generated reads do sit there (floors on the Python model's trace, which are
conditions on the inputs) and that the model and the C++ oracle agree on every one of them; the
GPU tests compare every device and host mapping route of libgfmatch with the oracle on those
reads, shuffled among ordinary ones.  Nothing here reads /root/reference.
"""
import functools

import numpy as np
import pytest

from oracle import indexer_model as M
from tests.gate_reads import gate_reads
from tests.helpers import matches_to_tuples

FLOOR = 20
CLASSES = (160, 256, 320)          # the flat pipeline's three instantiations: 10, 16 and 20 words per read


@functools.lru_cache(maxsize=None)
def _genes(which):
    from genefuserust_amd import synth
    if which == "clean":
        return synth.make_geneset("IDX-T", scale=0.05, repeat_frac=0.1)
    return synth.make_geneset("IDX-T", scale=0.3, repeat_frac=0.3, low_complexity_frac=0.05)  # test_repeat_rich_genes_parity


@functools.lru_cache(maxsize=None)
def _gate(which):
    return gate_reads(_genes(which).seqs, seed=2024 if which == "clean" else 2025, n=4000 if which == "clean" else 2000)


@functools.lru_cache(maxsize=None)
def _model(which):
    return M.IndexModel([s.decode() for s in _genes(which).seqs])


def _inner_stretches(mask, target):
    """Lengths of the stretches below `target` that lie between two bases equal to it, nothing above it between."""
    out, last = set(), None
    for j, m in enumerate(mask):
        if m > target:
            last = None
        elif m == target:
            if last is not None and j - last > 1:
                out.add(j - last - 1)
            last = j
    return out


def _describe(mx, family, read):
    t = mx.map_read_trace(read.decode())
    return "%-11s len %3d votes %s diagonals %s unmasked %s spans %s -> %s  %s" % (
        family, len(read), t.votes, t.diagonals, t.unmasked, t.spans, t.segments, read.decode())


def test_model_equals_oracle_and_reads_straddle_every_gate(oracle):
    """Clean index.  The floors are conditions on the inputs: were one missed, the family would have to be
    sharpened or enlarged, never the floor lowered."""
    mx, ox = _model("clean"), oracle.OracleIndexer(_genes("clean").seqs)
    reads = _gate("clean")
    assert 3500 <= len(reads) <= 4800
    lens = [len(r) for f, r in reads if f != "dupe"]
    assert min(lens) >= 98 and max(lens) <= 302
    assert all(50 <= len(r) <= 66 for f, r in reads if f == "dupe")
    assert all(sum(1 for n in lens if lo < n <= hi) > 300 for lo, hi in ((0, 160), (160, 256), (256, 320)))
    n = {}

    def hit(name):
        n[name] = n.get(name, 0) + 1

    for family, read in reads:
        t = mx.map_read_trace(read.decode())
        assert t.segments == ox.map_read(read), _describe(mx, family, read)
        c1, c2, c3 = t.votes
        if family == "dupe":   # (kept out of the floors below: those are about junction reads)
            # the stride-2 windows that vote at all: the least that "verified + still open" can come down to
            voting = sum(1 for i in range(0, len(read) - M.K + 1, 2) if mx.sites(M.kmer_at(read.decode(), i)))
            if voting in (18, 19) or (voting in (20, 21) and t.segments):
                hit("voting windows %d" % voting)
            continue
        if 18 <= c1 <= 22:
            hit("first %d" % c1)
        if c1 >= 20 and 8 <= c2 <= 12:
            hit("second %d" % c2)
        if t.mask is None:
            continue
        if c1 == c2:
            hit("first-place tie")
        if c2 == c3:
            hit("second-place tie")
        if 8 <= t.unmasked <= 13:
            hit("unmasked %d" % t.unmasked)
        if t.spans is None:
            continue
        if 19 <= t.spans[1] <= 22:
            hit("minor span %d" % t.spans[1])
        if 20 <= t.spans[0] <= 21:
            hit("major span %d" % t.spans[0])
        for g in (_inner_stretches(t.mask, 3) | _inner_stretches(t.mask, 2)) & {9, 10}:
            hit("inner stretch %d" % g)
        if len(t.segments) == 1:
            hit("one segment")
        if family == "indel1" and len(t.segments) == 2:
            hit("two segments after a 1-bp indel")
    floors = {"first %d" % v: FLOOR for v in (18, 19, 20, 21, 22)}
    floors.update({"second %d" % v: FLOOR for v in (8, 9, 10, 11, 12)})
    floors.update({"unmasked %d" % v: FLOOR for v in (8, 9, 10, 11, 12, 13)})
    floors.update({"minor span %d" % v: FLOOR for v in (19, 20, 21, 22)})
    floors.update({"voting windows %d" % v: FLOOR for v in (18, 19, 20, 21)})   # 20, 21: with a segment
    floors.update({"major span 21": FLOOR, "major span 20": 3, "inner stretch 9": FLOOR, "inner stretch 10": FLOOR,
                   "first-place tie": FLOOR, "second-place tie": FLOOR, "one segment": FLOOR,
                   "two segments after a 1-bp indel": FLOOR})
    print(sorted(n.items()))
    short = {k: (n.get(k, 0), v) for k, v in floors.items() if n.get(k, 0) < v}
    assert not short, short


def test_model_equals_oracle_next_to_repeats(oracle):
    """Repeat-rich index: the reads at a gate hold windows whose key has six sites or more, which is where the
    HIGH-flag and representative-site shortcut of the bucket pass works."""
    mx, ox = _model("rich"), oracle.OracleIndexer(_genes("rich").seqs)
    assert ox.stats()["n_high_keys"] > 200
    reads = _gate("rich")
    assert 1800 <= len(reads) <= 2200
    near = 0
    for family, read in reads:
        t = mx.map_read_trace(read.decode())
        assert t.segments == ox.map_read(read), _describe(mx, family, read)
        c1, c2, _ = t.votes
        at_vote_gate = abs(c1 - 20) <= 2 or (c1 >= 20 and abs(c2 - 10) <= 2)
        at_mask_gate = t.unmasked is not None and abs(t.unmasked - 10) <= 2
        if (at_vote_gate or at_mask_gate) and mx.high_windows(read.decode()) > 0:
            near += 1
    print("at a gate with a HIGH window:", near)
    assert near >= 100


# ---- the device and host routes of libgfmatch against the oracle (MI355X) ----

_FILL_MIX = "GATE_FILL"            # background and single-gene reads, no junctions: what surrounds a junction read in a run
_EXPECT = {}


@functools.lru_cache(maxsize=None)
def _gate_gpu(which):
    """About 4 000 gate reads on either index (the CPU test above walks 2 000 of the repeat-rich set's in Python)."""
    return _gate(which) if which == "clean" else gate_reads(_genes(which).seqs, seed=2026, n=4000)


@functools.lru_cache(maxsize=None)
def _batch(which, lo, hi, fill_len, dupes=False):
    """The gate reads longer than `lo` and at most `hi` bases, shuffled among three times as many filler reads of
    `fill_len` bases (so that waves, the LDS queue and the lists hold the usual mixture of lanes):
    (families, reads, bases, offsets).  `dupes`: with the short reads of the dupe family whatever the bounds (a batch's
    max_read_len chooses the instantiation, and only these reads make the first-place proof tight)."""
    from genefuserust_amd import synth
    gate = [(f, r) for f, r in _gate_gpu(which) if lo < len(r) <= hi or (dupes and f == "dupe")]
    synth.MIXES[_FILL_MIX] = (0.5, 0.5, 0.0)
    rb = synth.make_reads(_genes(which), 3 * len(gate), read_len=fill_len, mix=_FILL_MIX, seed=500 + fill_len)
    fill = rb.bases.numpy().reshape(-1, fill_len)
    both = gate + [("filler", row.tobytes()) for row in fill]
    order = np.random.default_rng(hi + fill_len).permutation(len(both))
    families, reads = [both[k][0] for k in order], [both[k][1] for k in order]
    bases, offsets = synth.ragged_batch(reads)
    return families, reads, bases, offsets


def _class_batch(which, cap):
    return _batch(which, {160: 0, 256: 160, 320: 256}[cap], cap, cap, dupes=True)


def _ragged_batch(which):
    """Every length class in one batch."""
    from genefuserust_amd import synth
    parts = [_class_batch(which, cap) for cap in CLASSES]
    families = [f for p in parts for f in p[0]]
    reads = [r for p in parts for r in p[1]]
    order = np.random.default_rng(7).permutation(len(reads))
    families, reads = [families[k] for k in order], [reads[k] for k in order]
    return (families, reads) + synth.ragged_batch(reads)


def _expected(oracle, which, key, bases, offsets):
    """OracleIndexer.map_reads_packed, once per batch."""
    if (which, key) not in _EXPECT:
        ox = oracle.OracleIndexer(_genes(which).seqs)
        _EXPECT[which, key] = ox.map_reads_packed(bases, offsets, threads=8)
        ox.close()
    return _EXPECT[which, key]


def _make_index(which):
    from genefuserust_amd import Indexer
    genes = _genes(which)
    ix = Indexer.from_gene_slices(genes.seqs, genes.reversed_flags)
    ix.make_index()
    return ix


def _host(counts, matches, n):
    """Device results as the host calls return them."""
    from genefuserust_amd import _lib
    import torch
    torch.cuda.synchronize()
    c = counts.cpu().numpy().astype(np.int32)[:n]
    m = matches.cpu().numpy().view(_lib.SEQMATCH_DTYPE).reshape(-1, 2)[:n]
    return c, m


def _compare(label, which, batch, got, want):
    """counts everywhere, the first match where there is one, the second where there are two.  Returns the lines of
    a failure report: the first reads that differ, with their family and the model's trace (none: all equal)."""
    families, reads = batch[0], batch[1]
    (counts, matches), (ocounts, omatches) = got, want
    assert counts.shape == ocounts.shape
    bad = counts != ocounts
    bad |= (ocounts > 0) & (matches[:, 0] != omatches[:, 0])
    bad |= (ocounts == 2) & (matches[:, 1] != omatches[:, 1])
    if not bad.any():
        return []
    rows = np.nonzero(bad)[0]
    mx = _model(which)
    lines = ["%s: %d of %d reads differ from the oracle" % (label, rows.size, counts.size)]
    for r in rows[:8]:
        lines.append("read %d got %s want %s\n    %s" % (
            r, matches_to_tuples(np.minimum(counts[r:r + 1], 2), matches[r:r + 1])[0] if counts[r] <= 2 else int(counts[r]),
            matches_to_tuples(ocounts[r:r + 1], omatches[r:r + 1])[0], _describe(mx, families[r], reads[r])))
    return lines


def _settle(problems):
    if problems:
        pytest.fail("\n".join(problems))


WHICH = ["clean", "rich"]


@pytest.mark.gpu
@pytest.mark.parametrize("bloom", ["default", "0", "1"])
@pytest.mark.parametrize("which", WHICH)
def test_flat_pipeline_ascii(gpu_device, oracle, which, bloom, monkeypatch):
    """map_reads_device, variant 0, one batch per length class, under the three filter builds."""
    import torch
    if bloom != "default":
        monkeypatch.setenv("GF_BLOOM_KIB", bloom)
    ix = _make_index(which)
    problems = []
    try:
        ix.set_map_variant(0)
        for cap in CLASSES:
            batch = _class_batch(which, cap)
            d_b, d_o = torch.from_numpy(batch[2]).cuda(), torch.from_numpy(batch[3]).cuda()
            got = _host(*ix.map_reads_device(d_b, d_o, cap), len(batch[1]))
            problems += _compare("flat pipeline, filter %s, class %d" % (bloom, cap), which, batch, got,
                                 _expected(oracle, which, cap, batch[2], batch[3]))
    finally:
        ix.close()
    _settle(problems)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("which", WHICH)
def test_exact_kernel(gpu_device, oracle, which, variant):
    """The wave-per-read kernel on one ragged batch, at its first two LDS footprints."""
    import torch
    ix = _make_index(which)
    problems = []
    try:
        ix.set_map_variant(variant)
        batch = _ragged_batch(which)
        want = _expected(oracle, which, "ragged", batch[2], batch[3])
        d_b, d_o = torch.from_numpy(batch[2]).cuda(), torch.from_numpy(batch[3]).cuda()
        for lcap in (320, 1024):
            got = _host(*ix.map_reads_device(d_b, d_o, lcap), len(batch[1]))
            problems += _compare("variant %d, max_read_len %d" % (variant, lcap), which, batch, got, want)
    finally:
        ix.set_map_variant(0)
        ix.close()
    _settle(problems)


@pytest.mark.gpu
@pytest.mark.parametrize("which", WHICH)
def test_packed_hand_over(gpu_device, oracle, which):
    """pack_bases_device, then map_reads_packed_device."""
    import torch
    ix = _make_index(which)
    problems = []
    try:
        for cap in (160, 320):
            batch = _class_batch(which, cap)
            d_b, d_o = torch.from_numpy(batch[2]).cuda(), torch.from_numpy(batch[3]).cuda()
            pk, iv = ix.pack_bases_device(d_b)
            got = _host(*ix.map_reads_packed_device(pk, iv, d_o, cap), len(batch[1]))
            problems += _compare("packed hand-over, class %d" % cap, which, batch, got,
                                 _expected(oracle, which, cap, batch[2], batch[3]))
    finally:
        ix.close()
    _settle(problems)


@pytest.mark.gpu
@pytest.mark.parametrize("which", WHICH)
def test_fixed_length_form(gpu_device, oracle, which):
    """map_reads_fixed_device on the gate reads of exactly 150 and exactly 300 bases."""
    import torch
    ix = _make_index(which)
    problems = []
    try:
        for L in (150, 300):
            batch = _batch(which, L - 1, L, L)
            assert len(batch[1]) > 800 and (np.diff(batch[3]) == L).all()
            got = _host(*ix.map_reads_fixed_device(torch.from_numpy(batch[2]).cuda(), L), len(batch[1]))
            problems += _compare("fixed length %d" % L, which, batch, got,
                                 _expected(oracle, which, "fixed%d" % L, batch[2], batch[3]))
    finally:
        ix.close()
    _settle(problems)


@pytest.mark.gpu
@pytest.mark.parametrize("route", [-1, 0])
def test_host_calls(gpu_device, oracle, route):
    """map_reads_packed in calls of at most 8 192 reads: the zero-copy route (-1, the default) and the batch route (0)."""
    which = "clean"
    ix = _make_index(which)
    problems = []
    try:
        ix.set_pack_call_reads(route)
        families, reads, bases, offsets = _ragged_batch(which)
        counts, matches = [], []
        for r0 in range(0, len(reads), 8192):
            r1 = min(r0 + 8192, len(reads))
            c, m = ix.map_reads_packed(bases[offsets[r0]:offsets[r1]], offsets[r0:r1 + 1] - offsets[r0])
            counts.append(c)
            matches.append(m)
        problems = _compare("host calls, route %d" % route, which, (families, reads),
                            (np.concatenate(counts), np.concatenate(matches)), _expected(oracle, which, "ragged", bases, offsets))
    finally:
        ix.set_pack_call_reads(-1)
        ix.close()
    _settle(problems)
