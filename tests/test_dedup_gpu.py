"""libgfdedup.so on the device (include/gf_dedup.h): keys, insert, rehash, remove and histogram against the model
(tests/dedup_model.py) — every array compared exactly — and every route of a scan with ``dedup``: whole file against
streamed, both against the model over the files, with a table that grows mid-stream."""
import os

import numpy as np
import pytest

from genefuserust_amd import dedup as dd
from tests import dedup_model as model
from tests.dedup_cases import LENGTHS, batch_pairs, batch_reads, edge_reads, swap_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 255, 256, 257, 600]


@pytest.fixture(scope="module")
def ix(gpu_device):
    from genefuserust_amd import Indexer
    index = Indexer.from_gene_slices([b"ACGT" * 64])
    index.make_index()
    yield index
    index.close()


def _up(x):
    import torch
    return torch.from_numpy(np.frombuffer(x, dtype=np.uint8).copy()).cuda()


def _batch_at(b: bytes, q: bytes, offsets):
    """A batch over the bytes ``b`` / ``q`` with the given offsets, which need neither start at 0 nor run forwards."""
    import torch
    from genefuserust_amd.fastq import FastqBatch
    none = torch.zeros(0, dtype=torch.int64, device="cuda")
    off = torch.from_numpy(np.asarray(offsets, dtype=np.int64)).cuda()
    return FastqBatch(_up(b), _up(q), off, len(offsets) - 1, none, 0, 0)


def _quals(r: bytes, salt: int) -> bytes:
    return bytes(33 + (salt + 7 * j) % 41 for j in range(len(r)))


def _batch(reads, lead: int = 0):
    """The records as the full FASTQ cut leaves them; ``lead`` bytes of another record in front of the first, so that
    the first byte of the records lies at that alignment."""
    off = lead + np.concatenate([[0], np.cumsum([len(r) for r in reads], dtype=np.int64)])
    return _batch_at(b"G" * lead + b"".join(reads), b"~" * lead + b"".join(_quals(r, k) for k, r in enumerate(reads)),
                     off)


def _u64(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def _key_tensor(keys):
    import torch
    return torch.from_numpy(np.asarray(keys, dtype=np.uint64).view(np.int64).copy()).cuda()


def _totals():
    import torch
    return torch.zeros(dd.TOTALS, dtype=torch.int64, device="cuda")


def _entries(table, counted=True):
    keys, first = _u64(table.keys), table.first.cpu().numpy()
    at = np.nonzero(keys)[0]
    assert (first[keys == 0] == dd.NO_INDEX).all()
    if table.count is None or not counted:
        return {(int(keys[s]), int(first[s])) for s in at}
    count = table.count.cpu().numpy().view(np.uint32)
    assert not count[keys == 0].any()
    return {(int(keys[s]), int(first[s]), int(count[s])) for s in at}


def _insert(ix, table, keys, first_index, totals):
    """One insert call; the records' slots point at the records' keys."""
    slot = dd.insert_device(ix, _key_tensor(keys), first_index, table, totals).cpu().numpy()
    stored = _u64(table.keys)
    for k, s in zip(keys, slot):
        assert (s == -1) if k == 0 else (0 <= s < table.slots and int(stored[s]) == k)
    return slot


# ---- keys ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_keys_of_every_edge_length_at_every_lead(ix):
    """Every length of the cases; over the set all 16 leads occur on both sides, the two sides at different ones."""
    reads = list(edge_reads())
    assert sorted({len(r) for r in reads}) == LENGTHS
    seen = set()
    for lead in range(16):
        other = (5 * lead + 3) % 16
        seen.add(other)
        assert other != lead
        mates = reads[::-1]
        got = _u64(dd.keys_device(ix, _batch(reads, lead), _batch(mates, other)))
        assert got.tolist() == [model.key(a, b) for a, b in zip(reads, mates)], lead
        single = _u64(dd.keys_device(ix, _batch(reads, lead)))
        assert single.tolist() == [model.key(r) for r in reads], lead
    assert seen == set(range(16))
    assert int(_u64(dd.keys_device(ix, _batch([b"ACGT"])))[0]) == 0xab0fcab10dd0c6f9
    assert int(_u64(dd.keys_device(ix, _batch([b"ACGT"], 3), _batch([b""], 9)))[0]) == 0xade372bd9e169438


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_keys_batch_sizes_and_empty_mates(ix, n):
    pairs = batch_pairs(n, salt=n)
    left, right = [a for a, _ in pairs], [b for _, b in pairs]
    got = _u64(dd.keys_device(ix, _batch(left, n % 16), _batch(right, (n + 7) % 16)))
    want = [model.key(a, b) for a, b in pairs]
    assert got.tolist() == want
    if n >= 255:
        assert want[5] == 0 and any(a and not b for a, b in pairs) and any(b and not a for a, b in pairs)
        assert len(set(want)) < len(want)   # repeats among the pairs


@pytest.mark.gpu
def test_keys_with_offsets_that_run_backwards(ix):
    reads = [r for r in edge_reads() if 0 < len(r) <= 300]
    lead, b = 5, b"".join(reads)
    off = [lead + int(x) for x in np.concatenate([[0], np.cumsum([len(r) for r in reads])])]
    j = next(k for k, r in enumerate(reads) if len(r) == 257)
    off[j + 1:j + 1] = [off[j] + 20, off[j] + 3]
    bb = b"G" * lead + b
    cut = [bb[s:max(s, e)] for s, e in zip(off, off[1:])]
    assert [len(x) for x in cut[j:j + 3]] == [20, 0, 254]
    got = _u64(dd.keys_device(ix, _batch_at(bb, b"F" * len(bb), off)))
    assert got.tolist() == [model.key(r) for r in cut] and got[j + 1] == 0


# ---- insert, with keys given directly -----------------------------------------------------------------------------------

def _distinct_keys(n, salt=0):
    return [model.mix(salt * 100_003 + k + 1) or 1 for k in range(n)]


@pytest.mark.gpu
def test_insert_equal_distinct_chained_and_repeated(ix):
    slots = 1024
    # 600 equal keys: one entry, the lowest index, count 600 (past half full is the caller's business, not the call's)
    table, totals, t = dd.empty_table(slots, "cuda"), _totals(), model.Table()
    keys = [0xab0fcab10dd0c6f9] * 600
    _insert(ix, table, keys, 40, totals)
    want = t.insert(keys, 40)
    assert _entries(table) == t.entries() == {(keys[0], 40, 600)} and totals.cpu().tolist() == want
    # 600 distinct keys in a table of 4096, a few of them 0
    table, totals, t = dd.empty_table(4096, "cuda"), _totals(), model.Table()
    keys = _distinct_keys(600)
    keys[17] = keys[300] = 0
    _insert(ix, table, keys, 0, totals)
    assert totals.cpu().tolist() == t.insert(keys, 0) == [600, 598, 598, 0, 0, 0]
    assert _entries(table) == t.entries() and len(t.entries()) == 598
    # the same batch offered again behind itself: all duplicates
    slot = _insert(ix, table, keys, 600, totals)
    more = t.insert(keys, 600)
    assert totals.cpu().tolist() == [1200, 1196, 598, 0, 0, 0] and more[2] == 0
    assert _entries(table) == t.entries() and {c for _, _, c in t.entries()} == {2}
    first = table.first.cpu().numpy()
    assert all(first[s] != 600 + i for i, s in enumerate(slot) if s >= 0)
    # a batch with a lower first_index than an earlier one: first is the minimum
    table, totals, t = dd.empty_table(slots, "cuda"), _totals(), model.Table()
    keys = _distinct_keys(300, salt=1)
    for first_index in (5000, 100, 700):
        _insert(ix, table, keys, first_index, totals)
        t.insert(keys, first_index)
    assert _entries(table) == t.entries() == {(k, 100 + i, 3) for i, k in enumerate(keys)}


@pytest.mark.gpu
def test_insert_one_chain_that_wraps_in_a_half_full_table(ix):
    slots = 1024
    chain = [(k << 10) | 1023 for k in range(1, 513)]
    assert {model.home(k, slots) for k in chain} == {1023}
    for counted in (True, False):
        table, totals, t = dd.empty_table(slots, "cuda", counted), _totals(), model.Table()
        _insert(ix, table, chain, 7, totals)
        assert totals.cpu().tolist() == t.insert(chain, 7) == [512, 512, 512, 0, 0, 0]   # every key placed, none failed
        assert _entries(table, counted) == t.entries(counted)
        occupied = np.nonzero(_u64(table.keys))[0]
        assert occupied.tolist() == list(range(511)) + [1023]   # the chain wraps
        # with count NULL the set of (key, first) is as before
        _insert(ix, table, chain[::-1], 1000, totals)
        t.insert(chain[::-1], 1000)
        assert _entries(table, counted) == t.entries(counted) and totals.cpu().tolist()[5] == 0


# ---- rehash -------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_rehash_keeps_the_set_and_later_inserts_find_the_old_keys(ix):
    import torch
    old, totals, t = dd.empty_table(1024, "cuda"), _totals(), model.Table()
    keys = [(k << 10) | 1023 for k in range(1, 201)] + _distinct_keys(300, salt=2)
    _insert(ix, old, keys + keys[:50], 0, totals)
    t.insert(keys + keys[:50], 0)
    new = dd.Table(torch.full((4096,), 77, dtype=torch.int64, device="cuda"),       # (the call empties it)
                   torch.full((4096,), 77, dtype=torch.int64, device="cuda"),
                   torch.full((4096,), 77, dtype=torch.int32, device="cuda"))
    dd.rehash_device(ix, old, new)
    assert _entries(new) == _entries(old) == t.entries() and len(t.entries()) == 500
    again = keys[100:400] + _distinct_keys(40, salt=3)
    _insert(ix, new, again, 550, totals)
    added = t.insert(again, 550)
    assert added[2] == 40 and totals.cpu().tolist()[2] == 540 and _entries(new) == t.entries()


# ---- remove -------------------------------------------------------------------------------------------------------------

def _cut(batch):
    off = batch.offsets.cpu().numpy()
    b, q = batch.bases.cpu().numpy().tobytes(), batch.quals.cpu().numpy().tobytes()
    return [(b[s:e], q[s:e]) for s, e in zip(off, off[1:])], off


def _remove_against_the_model(ix, table, t, pairs, leads, totals=None):
    """Keys, insert and remove of ``pairs`` (reads when the mates are None) behind what ``table`` already holds."""
    single = pairs and pairs[0][1] is None
    sides = [[a for a, _ in pairs]] + ([] if single else [[b for _, b in pairs]])
    batches = [_batch(side, lead) for side, lead in zip(sides, leads)]
    first_index, totals = t.offered, _totals() if totals is None else totals
    before = totals.cpu().tolist()
    rec_keys = dd.keys_device(ix, *batches)
    rec_slot = dd.insert_device(ix, rec_keys, first_index, table, totals)
    *out, dup = dd.remove_device(ix, rec_slot, first_index, table, totals, *batches)
    want = t.offer([a if single else (a, b) for a, b in pairs], first_index)
    assert dup.cpu().numpy().tolist() == want.dup
    assert [g - b for g, b in zip(totals.cpu().tolist(), before)] == want.totals
    for side, batch in zip(sides, out):
        got, off = _cut(batch)
        assert off[0] == 0 and batch.qual_off is None
        assert got == [(b"", b"") if d else (r, _quals(r, k)) for k, (r, d) in enumerate(zip(side, want.dup))]
    assert _entries(table) == t.entries()
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_remove_against_the_model(ix, n):
    table, t = dd.empty_table(4096, "cuda"), model.Table()
    want = _remove_against_the_model(ix, table, t, batch_pairs(n, salt=n), (n % 16, (n + 7) % 16))
    if n >= 255:
        assert 0 < want.totals[3] < want.totals[1] < want.totals[0] == n and want.totals[4] > 0
    # a second batch behind it: duplicates of the first batch's records, too; single-end in a table of its own
    more = _remove_against_the_model(ix, table, t, batch_pairs(n, salt=n)[::2], (3, 12))
    assert more.totals[2] == 0 and more.totals[3] == more.totals[1]
    reads = [(r, None) for r in batch_reads(n, salt=n)]
    _remove_against_the_model(ix, dd.empty_table(1024, "cuda"), model.Table(), reads, ((5 * n) % 16,))


@pytest.mark.gpu
def test_remove_everything_and_nothing(ix):
    read = edge_reads()[30]
    copies = [(read if k % 3 else swap_case(read), read[::-1]) for k in range(300)]
    want = _remove_against_the_model(ix, dd.empty_table(1024, "cuda"), model.Table(), copies, (1, 2))
    assert want.dup == [0] + [1] * 299 and want.totals == [300, 300, 1, 299, 299 * 2 * len(read), 0]
    rng = np.random.default_rng(8)
    distinct = [(bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 40)), b"AC") for _ in range(300)]
    want = _remove_against_the_model(ix, dd.empty_table(1024, "cuda"), model.Table(), distinct, (6, 11))
    assert not any(want.dup) and want.totals == [300, 300, 300, 0, 0, 0]


# ---- indices past 32 bits, a table with no room, a rehash without counts ------------------------------------------------

BIG_INDEX = (1 << 40) + 7


def _distinct_reads(rng, n, shortest, longest):
    reads = set()
    while len(reads) < n:
        reads.add(bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(rng.integers(shortest, longest + 1)))))
    return sorted(reads)


def _offer_at(ix, table, t, reads, first_index, lead=0):
    """Keys, insert and remove of single-end ``reads`` at ``first_index``, with totals of their own: duplicate flags,
    totals and the records that leave against the model.  Returns (the model's answer, the records' slots)."""
    batch, totals = _batch(reads, lead), _totals()
    rec_keys = dd.keys_device(ix, batch)
    assert _u64(rec_keys).tolist() == [model.key(r) for r in reads]
    rec_slot = dd.insert_device(ix, rec_keys, first_index, table, totals)
    out, dup = dd.remove_device(ix, rec_slot, first_index, table, totals, batch)
    want = t.offer(reads, first_index)
    assert dup.cpu().numpy().tolist() == want.dup
    assert totals.cpu().tolist() == want.totals
    got, off = _cut(out)
    assert off[0] == 0
    assert got == [(b"", b"") if d else (r, _quals(r, k)) for k, (r, d) in enumerate(zip(reads, want.dup))]
    return want, rec_slot.cpu().numpy()


@pytest.mark.gpu
def test_first_index_past_32_bits(ix):
    """``first`` is a 64-bit minimum and is compared as one: a batch at 2^40 + 7, then the same keys at 2^40 - 300.  The
    two indices of a key differ above and below bit 32; every ``first_index`` elsewhere is at most 5000."""
    rng = np.random.default_rng(12)
    reads = _distinct_reads(rng, 500, 20, 60)
    reads = reads + reads[100:200] + [b""]                    # repeats inside the batch, and a record without bases
    table, t = dd.empty_table(4096, "cuda"), model.Table()
    want, _ = _offer_at(ix, table, t, reads, BIG_INDEX, lead=3)
    assert want.totals[:4] == [601, 600, 500, 100] and _entries(table) == t.entries()
    assert {f for _, f, _ in t.entries()} == {BIG_INDEX + i for i in range(500)}
    lower = (1 << 40) - 300
    want, _ = _offer_at(ix, table, t, reads, lower, lead=9)
    assert want.totals[:4] == [601, 600, 0, 100]              # only the repeats inside the batch: every first is this call's
    assert _entries(table) == t.entries()
    assert t.entries() == {(model.key(r), lower + i, 4 if 100 <= i < 200 else 2) for i, r in enumerate(reads[:500])}
    # a third call above both: every record with bases is a duplicate
    want, _ = _offer_at(ix, table, t, reads, BIG_INDEX + 5000)
    assert want.totals[2:4] == [0, 600] and _entries(table) == t.entries()


@pytest.mark.gpu
def test_a_table_with_no_room(ix):
    """1024 distinct keys fill a table of 1024 slots exactly.  Of a second call's 100 new keys none finds room: no slot,
    counted in totals [5], never a duplicate, the bytes kept; its 200 old keys are found.  The table changes in the counts
    of those 200 alone."""
    slots = 1024
    rng = np.random.default_rng(13)
    old = _distinct_reads(rng, slots, 20, 40)
    new = _distinct_reads(rng, 100, 41, 50)
    table, t = dd.empty_table(slots, "cuda"), model.Table(slots=slots)
    want, slot = _offer_at(ix, table, t, old, 0, lead=5)
    assert want.totals == [slots, slots, slots, 0, 0, 0] and sorted(slot.tolist()) == list(range(slots))
    before = _entries(table)
    assert before == t.entries() and len(before) == slots
    again = [old[int(k)] for k in rng.choice(slots, 200, replace=False)]
    mixed = [(new + again)[int(k)] for k in rng.permutation(300)]
    is_new = np.array([len(r) > 40 for r in mixed])
    want, slot = _offer_at(ix, table, t, mixed, slots, lead=11)
    assert want.totals == [300, 300, 0, 200, sum(len(r) for r in again), 100]
    assert (slot[is_new] == -1).all() and (slot[~is_new] >= 0).all() and (slot[~is_new] < slots).all()
    stored = _u64(table.keys)
    assert [int(stored[s]) for s in slot[~is_new]] == [model.key(r) for r, n in zip(mixed, is_new) if not n]
    assert not any(d for d, n in zip(want.dup, is_new) if n) and all(d for d, n in zip(want.dup, is_new) if not n)
    found = {model.key(r) for r in again}
    assert _entries(table) == t.entries() == {(k, f, c + (k in found)) for k, f, c in before}


@pytest.mark.gpu
@pytest.mark.parametrize("old_counted,new_counted", [(True, False), (False, True)])
def test_rehash_between_a_counted_and_an_uncounted_table(ix, old_counted, new_counted):
    """The set of (key, first) is kept; the side that has no counts is not touched, and the old table stays as it is."""
    import torch
    old, totals, t = dd.empty_table(1024, "cuda", old_counted), _totals(), model.Table()
    keys = [(k << 10) | 1023 for k in range(1, 201)] + _distinct_keys(300, salt=6)
    _insert(ix, old, keys + keys[:50], 3, totals)
    t.insert(keys + keys[:50], 3)
    held = [None if x is None else x.clone() for x in old]
    new = dd.Table(torch.full((4096,), 77, dtype=torch.int64, device="cuda"),       # (the call empties it)
                   torch.full((4096,), 77, dtype=torch.int64, device="cuda"),
                   torch.full((4096,), 77, dtype=torch.int32, device="cuda") if new_counted else None)
    dd.rehash_device(ix, old, new)
    assert _entries(new, counted=False) == _entries(old, counted=False) == t.entries(False) and len(t.entries()) == 500
    for x, x0 in zip(old, held):
        assert (x is None and x0 is None) or torch.equal(x, x0)
    if new_counted:   # emptied, and nothing to add from
        assert not bool(new.count.any())
    else:
        assert _entries(old) == t.entries()
    # later inserts find the old keys
    again = keys[100:400] + _distinct_keys(40, salt=7)
    _insert(ix, new, again, 900, totals)
    added = t.insert(again, 900)
    assert added[2] == 40 and _entries(new, counted=False) == t.entries(False) and totals.cpu().tolist()[5] == 0


# ---- histogram ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_histogram_levels_and_accumulation(ix):
    import torch
    table, totals, t = dd.empty_table(1024, "cuda"), _totals(), model.Table()
    keys = []
    for k, times in enumerate([1, 2, 30, 31, 32, 100, 1, 1, 2]):
        keys += [_distinct_keys(9, salt=4)[k]] * times
    _insert(ix, table, keys, 0, totals)
    t.insert(keys, 0)
    want = t.histogram()
    assert [want[c] for c in (0, 1, 2, 30, 31)] == [0, 3, 2, 1, 3] and sum(want) == 9
    hist = torch.zeros(dd.LEVELS, dtype=torch.int64, device="cuda")
    dd.histogram_device(ix, table, hist)
    assert hist.cpu().tolist() == want
    dd.histogram_device(ix, table, hist)   # it adds
    assert hist.cpu().tolist() == [2 * x for x in want]


# ---- every route --------------------------------------------------------------------------------------------------------

CHUNK = 60_000


def _records(path):
    lines = open(path, "rb").read().split(b"\n")
    return [lines[k:k + 4] for k in range(0, len(lines) - (len(lines) % 4), 4)]


def _write(path, records, final_newline):
    with open(path, "wb") as f:
        f.write(b"\n".join(b"\n".join(r) for r in records) + (b"\n" if final_newline else b""))


@pytest.fixture(scope="module")
def files(tmp_path_factory, gpu_device):
    """The three pairs of tests/golden/R1.fq / R2.fq and, so that the scans have matches, the planted pairs of
    tests.test_adapter_trim_gpu._trimmed_files, with records repeated: some copies adjacent, three whole copies of the
    file behind it, every third copy in the other case.  A copy's name ends in " copyN"."""
    from tests.test_adapter_trim_gpu import _trimmed_files
    tmp = tmp_path_factory.mktemp("dedup_routes")
    f = _trimmed_files(tmp)
    golden = os.path.join(ROOT, "tests", "golden")
    firsts = [_records(os.path.join(golden, "R1.fq")) + _records(f["r1"]),
              _records(os.path.join(golden, "R2.fq")) + _records(f["r2"])]
    n = len(firsts[0])
    assert n == len(firsts[1]) == 153
    order, copies = [], 0
    for k in range(n):
        order.append((k, 0))
        if k % 10 == 0:
            copies += 1
            order.append((k, copies))
    for _ in range(3):
        for k in range(n):
            copies += 1
            order.append((k, copies))
    sides = []
    for side in firsts:
        out = []
        for k, c in order:
            name, seq, plus, qual = side[k]
            out.append([name + (b" copy%d" % c if c else b""), swap_case(seq) if c % 3 == 1 else seq, plus, qual])
        sides.append(out)
    f["n"], f["order"] = len(order), order
    for key, side, first, nl in (("r1", sides[0], firsts[0], True), ("r2", sides[1], firsts[1], False)):
        f["d" + key] = str(tmp / ("D%s.fq" % key))      # with the copies
        f["u" + key] = str(tmp / ("U%s.fq" % key))      # the first copies alone
        _write(f["d" + key], side, nl)
        _write(f["u" + key], first, nl)
    f["sides"] = [[(r[1], r[3]) for r in side] for side in sides]
    f["second"] = [[(r[1], r[3]) for r in side[::-1][:200]] for side in sides]
    for key, side, nl in (("s1", sides[0][::-1][:200], True), ("s2", sides[1][::-1][:200], False)):
        f[key] = str(tmp / (key + ".fq"))
        _write(f[key], side, nl)
    two = tmp / "two.txt"
    two.write_text("%s\n%s\n" % (f["csvs"][3], f["csvs"][0]))
    f["two"] = str(two)
    return f


def _model_result(record_lists, remove=True):
    """The ``DedupResult`` of one ``Dedup`` over the record lists (reads, or pairs of them), offered one after the other."""
    t, sums = model.Table(), [0] * 6
    for records in record_lists:
        sums = [a + b for a, b in zip(sums, t.offer(records).totals)]
    return dd.DedupResult(sums[1], sums[2], sums[3], sums[4] if remove else 0, tuple(t.histogram()))


def _pairs_of(sides):
    return [(a[0], b[0]) for a, b in zip(*sides)]


def _counters_of(result):
    return dict(zip(dd.DEDUP_COUNTER_KEYS, result[:4]))


def _first_copies_only(matches):
    assert len(matches) > 0 and not any(b" copy" in m.m_name for m in matches)
    return sorted(m.m_name for m in matches)


def _same_tables(a, b):
    assert len(a.after) == len(b.after)
    for x, y in zip(a.before + a.after, b.before + b.after):
        assert np.array_equal(x, y)


@pytest.mark.gpu
def test_pair_routes_whole_file_and_streamed(files):
    from genefuserust_amd.read_qc import ReadQc
    from genefuserust_amd.scan import scan_pair_end_files
    f = files
    args = (f["fa"], f["csvs"][3], f["dr1"], f["dr2"])
    want = _model_result([_pairs_of(f["sides"])])
    # (two of the golden pairs are copies of each other as they come)
    assert want.checked == f["n"] == 628 and want.unique == 152 and want.duplicates == 476 and want.histogram[4] > 100
    unique = scan_pair_end_files(f["fa"], f["csvs"][3], f["ur1"], f["ur2"])
    whole, streamed = dd.Dedup(slots=1024), dd.Dedup(slots=1024)
    qcs = ReadQc(), ReadQc()
    got = scan_pair_end_files(*args, dedup=whole, qc=qcs[0])
    got_streamed = scan_pair_end_files(*args, dedup=streamed, qc=qcs[1], chunk_bytes=CHUNK)
    assert got_streamed[1].pop("chunks") >= 3 and streamed.slots == 2048 and whole.slots == 2048   # it grew mid-stream
    assert got == got_streamed
    assert whole.result() == streamed.result() == want
    _same_tables(qcs[0].result(), qcs[1].result())
    assert qcs[0].result().summary("after")["total_reads"] == 2 * 152 < qcs[0].result().summary("before")["total_reads"]
    assert {k: got[1][k] for k in dd.DEDUP_COUNTER_KEYS} == _counters_of(want)
    keys = list(got[1])
    assert tuple(keys[keys.index("dedup_checked"):][:5]) == dd.DEDUP_COUNTER_KEYS + ("complexity",)
    # every match is named after the first copy, and they are the matches of the file without the copies
    assert _first_copies_only(got[0]) == sorted(m.m_name for m in unique[0])
    plain = scan_pair_end_files(*args)
    assert len(plain[0]) > len(got[0])
    # remove=False: the scan of the file as it is, and the same counts but for the bases
    count_only = dd.Dedup(remove=False, slots=1024)
    counted = scan_pair_end_files(*args, dedup=count_only, chunk_bytes=CHUNK)
    assert counted[0] == plain[0]
    assert {k: v for k, v in counted[1].items() if k not in dd.DEDUP_COUNTER_KEYS + ("chunks",)} == plain[1]
    assert {k: counted[1][k] for k in dd.DEDUP_COUNTER_KEYS} == dict(_counters_of(want), dedup_bases_removed=0)
    assert count_only.result() == want._replace(bases_removed=0)


@pytest.mark.gpu
def test_pair_routes_behind_trimming_and_filter(files):
    """The keys are those of the trimmed and filtered records: the model's trimming and filter in front of the model."""
    from genefuserust_amd.read_filter import ReadFilter
    from genefuserust_amd.scan import scan_pair_end_files
    from tests.adapter_trim_model import trim_batch
    from tests.read_filter_model import filter_batch
    from tests.test_adapter_trim_gpu import ROUTE_SETTINGS, _route_config
    f = files
    trimmed = trim_batch(f["sides"][0], f["sides"][1], ROUTE_SETTINGS)
    kept = filter_batch(trimmed.reads[0], trimmed.reads[1], f["fs"])
    want = _model_result([_pairs_of(kept.reads)])
    assert 0 < want.checked < f["n"] and want.duplicates > 200
    args = (f["fa"], f["csvs"][3], f["dr1"], f["dr2"])
    ahead = dict(adapter_trim=_route_config(), read_filter=ReadFilter(*f["fs"]))
    whole, streamed = dd.Dedup(slots=1024), dd.Dedup(slots=1024)
    got = scan_pair_end_files(*args, **ahead, dedup=whole)
    got_streamed = scan_pair_end_files(*args, **ahead, dedup=streamed, chunk_bytes=CHUNK)
    assert got_streamed[1].pop("chunks") >= 3 and got == got_streamed
    assert whole.result() == streamed.result() == want
    keys = list(got[1])
    at = keys.index("reads_mate_failed")
    assert tuple(keys[at + 1:at + 6]) == dd.DEDUP_COUNTER_KEYS + ("complexity",)
    unique = scan_pair_end_files(f["fa"], f["csvs"][3], f["ur1"], f["ur2"], **ahead)
    assert _first_copies_only(got[0]) == sorted(m.m_name for m in unique[0])


@pytest.mark.gpu
def test_single_end_routes(files):
    from genefuserust_amd.scan import scan_single_end_files
    f = files
    want = _model_result([[a[0] for a in f["sides"][0]]])
    assert want.unique == 152
    unique = scan_single_end_files(f["fa"], f["csvs"][3], f["ur1"])
    results = []
    for kwargs in (dict(route="device"), dict(route="host"), dict(chunk_bytes=CHUNK)):
        d = dd.Dedup(slots=1024)
        got = scan_single_end_files(f["fa"], f["csvs"][3], f["dr1"], **kwargs, dedup=d)
        got[1].pop("chunks", None)
        got[1].pop("retried_reads", None)   # (the host route does not count them)
        assert d.result() == want and _first_copies_only(got[0]) == sorted(m.m_name for m in unique[0])
        assert {k: got[1][k] for k in dd.DEDUP_COUNTER_KEYS} == _counters_of(want)
        results.append(got)
    assert results[0] == results[1] == results[2]


@pytest.mark.gpu
def test_two_csvs_are_deduplicated_once(files):
    from genefuserust_amd.multi_csv_scan import scan_multi_csv_report
    f = files
    want = _model_result([_pairs_of(f["sides"])])
    outs = []
    for chunk_bytes in (CHUNK, None):
        d = dd.Dedup(slots=1024)
        got = scan_multi_csv_report(f["fa"], f["two"], f["dr1"], f["dr2"], chunk_bytes=chunk_bytes, dedup=d)
        assert len(got) == 2 and d.result() == want and d.offered == f["n"]
        for _, _, counters in got:
            counters.pop("chunks", None)
            assert {k: counters[k] for k in dd.DEDUP_COUNTER_KEYS} == _counters_of(want)
        outs.append(got)
    assert outs[0] == outs[1]
    unique = scan_multi_csv_report(f["fa"], f["two"], f["ur1"], f["ur2"])
    assert [(c, r) for c, r, _ in outs[0]] == [(c, r) for c, r, _ in unique] and len(unique[0][1]) > 0


@pytest.mark.gpu
def test_one_dedup_over_two_scans(files):
    """The second file's records are duplicates of the first's wherever they repeat them: the model over the
    concatenation.  The same file twice: every record of the second pass is removed."""
    from genefuserust_amd.scan import scan_pair_end_files
    f = files
    d = dd.Dedup(slots=1024)
    scan_pair_end_files(f["fa"], f["csvs"][3], f["dr1"], f["dr2"], dedup=d, chunk_bytes=CHUNK)
    second = scan_pair_end_files(f["fa"], f["csvs"][3], f["s1"], f["s2"], dedup=d)
    assert d.result() == _model_result([_pairs_of(f["sides"]), _pairs_of(f["second"])])
    assert second[0] == [] and second[1]["dedup_unique"] == 0 and second[1]["dedup_duplicates"] == 200
    assert d.offered == f["n"] + 200


@pytest.mark.gpu
def test_a_second_device_a_full_table_and_a_lean_cut_are_refused(ix):
    import torch
    d = dd.Dedup(slots=1024, max_slots=1024)
    b = _batch(batch_reads(300))
    (out,), totals = d.apply(ix, b)
    assert d.result().checked == int(totals.cpu()[1]) and d.offered == 300
    with pytest.raises(RuntimeError, match="max_slots is 1024"):
        d.apply(ix, b)
    with pytest.raises(ValueError, match="full FASTQ cut"):
        dd.Dedup(slots=1024).apply(ix, b._replace(qual_off=b.offsets))

    class _Elsewhere:
        def info(self):
            return {"device": torch.cuda.current_device() + 1}
    with pytest.raises(ValueError, match="one of its own"):
        d.apply(_Elsewhere(), b)
