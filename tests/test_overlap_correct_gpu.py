"""libgfcorrect.so on the device (include/gf_overlap_correct.h): the kernel against the model of the predicate
(tests/overlap_correct_model.py) — bases and qualities of both sides, I*, the corrected bases per read and the totals,
all exact — every pair route with ``overlap_correct`` set against the model in front of the plain scan (the model's
output written as FASTQ files and scanned without the keyword), and what the correction is for: pairs with three
low-quality miscalls in the overlap merge, and PCR copies that differ by such a miscall are duplicates."""
import functools

import numpy as np
import pytest

from tests.adapter_trim_cases import bases_of, other_base, rc, read_through
from tests.adapter_trim_model import TOTAL_KEYS as TRIM_TOTAL_KEYS
from tests.adapter_trim_model import TRUSEQ_R1, TRUSEQ_R2
from tests.adapter_trim_model import Settings as TrimSettings
from tests.adapter_trim_model import trim_batch
from tests.overlap_correct_cases import SETTINGS, cases, modelled
from tests.overlap_correct_model import TOTAL_KEYS, Settings, correct_batch, insert_of
from tests.test_multi_csv_scan import _files

NEW_KEYS = TOTAL_KEYS[1:]
TRIM_KEYS = TRIM_TOTAL_KEYS[1:]
RF_KEYS = ("reads_passed", "reads_trimmed", "bases_trimmed", "reads_too_short", "reads_too_many_n",
           "reads_low_quality", "reads_mate_failed")
LEAD = (3, 9)


@pytest.fixture(scope="module")
def ix(gpu_device):
    from genefuserust_amd import Indexer
    index = Indexer.from_gene_slices([b"ACGT" * 64])
    index.make_index()
    yield index
    index.close()


def _config(s: Settings):
    from genefuserust_amd.overlap_correct import OverlapCorrect
    return OverlapCorrect(*s)


def _batch(reads, lead: int = 0):
    """The records as the full FASTQ cut leaves them; ``lead`` bytes of another record in front of the first."""
    import torch
    from genefuserust_amd.fastq import FastqBatch
    b = b"G" * lead + b"".join(r[0] for r in reads)
    q = b"~" * lead + b"".join(r[1] for r in reads)
    off = lead + np.concatenate([[0], np.cumsum([len(r[0]) for r in reads], dtype=np.int64)]).astype(np.int64)
    up = lambda x: torch.from_numpy(np.frombuffer(x, dtype=np.uint8).copy()).cuda()   # noqa: E731
    none = torch.zeros(0, dtype=torch.int64, device="cuda")
    return FastqBatch(up(b), up(q), torch.from_numpy(off).cuda(), len(reads), none, 0, 0)


def _bytes(t) -> bytes:
    return t.cpu().numpy().tobytes()


def _held_to_the_model(ix, s: Settings, picked, answers, lead=LEAD, inplace=False):
    """One call over the cases ``picked``; everything it leaves equals the model's, byte for byte, the lead bytes are as
    they were, and the caller's tensors are untouched (or, in place, hold the result).  Returns the model's answer."""
    from genefuserust_amd.overlap_correct import correct_overlaps_device
    left, right = [c[:2] for c in picked], [c[2:] for c in picked]
    given = [_batch(left, lead[0]), _batch(right, lead[1])]
    before = [(_bytes(b.bases), _bytes(b.quals), _bytes(b.offsets)) for b in given]
    l, r, totals, insert, fixed = correct_overlaps_device(ix, _config(s), *given, detail=True, inplace=inplace)
    want = correct_batch(left, right, s, answers)
    for k, (b, g, reads) in enumerate(zip((l, r), given, want.reads)):
        assert b.n_records == len(reads) and b.qual_off is None and _bytes(b.offsets) == before[k][2]
        assert _bytes(b.bases) == (b"G" * lead[k]) + b"".join(x[0] for x in reads)
        assert _bytes(b.quals) == (b"~" * lead[k]) + b"".join(x[1] for x in reads)
        if inplace:
            assert b.bases.data_ptr() == g.bases.data_ptr() and b.quals.data_ptr() == g.quals.data_ptr()
        else:
            assert (_bytes(g.bases), _bytes(g.quals), _bytes(g.offsets)) == before[k]
            assert len(picked) == 0 or b.bases.data_ptr() != g.bases.data_ptr()
    assert insert.cpu().numpy().tolist() == want.insert
    assert fixed.cpu().numpy().tolist() == want.fixed
    assert totals.cpu().numpy().tolist() == want.totals
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SETTINGS))
def test_kernel_against_the_model(ix, name):
    """All cases, more than a tile; the two sides at different alignments."""
    picked = cases(name)
    assert len(picked) > 256
    want = _held_to_the_model(ix, SETTINGS[name], picked, modelled(name))
    assert all(t > 0 for t in want.totals)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 600])
def test_batch_sizes(ix, n):
    """One pair, one tile, the tile's edges, and a partial third tile: the cases again and again, each at another
    place."""
    picked, answers = cases("defaults"), modelled("defaults")
    at = [(7 * n + k) % len(picked) for k in range(n)]
    _held_to_the_model(ix, SETTINGS["defaults"], [picked[k] for k in at], [answers[k] for k in at])


@pytest.mark.gpu
def test_degenerate_inputs(ix):
    """No pair, pairs of empty records, and pairs too short for any candidate: nothing is found, nothing changes."""
    from tests.overlap_correct_model import correct_pair
    rng = np.random.default_rng(9)
    s = Settings()
    short = [(bases_of(rng, int(L)), b"#" * int(L), bases_of(rng, int(M)), b"I" * int(M))
             for L, M in rng.integers(20, 29, (300, 2)).tolist()]
    for picked in ([], [(b"", b"", b"", b"")] * 3, short):
        answers = [correct_pair(*c, s) for c in picked]
        want = _held_to_the_model(ix, s, picked, answers, lead=(7, 11))
        assert want.totals == [len(picked), 0, 0, 0, 0, 0]


@pytest.mark.gpu
def test_the_callers_buffers(ix):
    """``inplace=False`` leaves the tensors it was given as they were; ``inplace=True`` writes the result into them; the
    bytes in front of the first record never change (``_held_to_the_model`` asserts all three)."""
    picked, answers = cases("defaults"), modelled("defaults")
    for inplace in (False, True):
        want = _held_to_the_model(ix, SETTINGS["defaults"], picked, answers, lead=(5, 16), inplace=inplace)
        assert want.totals[4] > 0


# ---- every route ------------------------------------------------------------------------------------------------------

CHUNK = 12_000
ROUTE_SETTINGS = Settings()
ROUTE_TRIM = TrimSettings(adapter_r1=TRUSEQ_R1, adapter_r2=TRUSEQ_R2)


def _records(path):
    lines = open(path, "rb").read().split(b"\n")
    return [lines[k:k + 4] for k in range(0, len(lines) - 3, 4)]


def _write(path, records, final_newline):
    open(path, "wb").write(b"\n".join(b"\n".join(r) for r in records) + (b"\n" if final_newline else b""))


def _miscall(rec, at: int, q: int):
    """The base at ``at`` of the FASTQ record flipped, with the quality byte ``q``."""
    bases, quals = bytearray(rec[1]), bytearray(rec[3])
    if bytes(bases[at:at + 1]).upper() in (b"A", b"C", b"G", b"T"):
        bases[at] = other_base(bases[at])
    quals[at] = q
    rec[1], rec[3] = bytes(bases), bytes(quals)


@pytest.fixture(scope="module")
def corrected_files(tmp_path_factory):
    return _corrected_files(tmp_path_factory.mktemp("overlap_correct_routes"))


def _corrected_files(tmp):
    """tests.test_multi_csv_scan._files with low-quality miscalls planted inside the overlaps of the pairs that carry a
    fusion (k % 3 != 2), in either mate, and now and then a miscall of good quality beside them; every fifth pair also
    gets the read-through of tests.test_adapter_trim_gpu._trimmed_files first.  Beside them the model's output as files
    (m1.fq / m2.fq), and with the trimming's model and then the read filter's behind it (f1.fq / f2.fq)."""
    from tests.read_filter_model import Settings as FilterSettings
    from tests.read_filter_model import filter_batch
    fa, lst, csvs, r1, r2 = _files(tmp)
    rng = np.random.default_rng(41)
    s = ROUTE_SETTINGS
    sides = [_records(r1), _records(r2)]
    for k in range(len(sides[0])):
        l, r = sides[0][k], sides[1][k]
        if k % 5 == 0:   # a fragment of the first 95 to 140 bases of R1, read through by both mates
            l[1], r[1] = read_through(rng, l[1][:int(rng.integers(95, 141))], 150, 150, ROUTE_TRIM)
            l[3], r[3] = b"F" * 150, b"F" * 150
        insert = insert_of(l[1], r[1], s)
        if k % 3 == 2 or insert < 0:
            continue
        lo, hi = max(0, insert - len(r[1])), min(insert, len(l[1]))
        where = [int(x) for x in rng.choice(np.arange(lo, hi), 1 + k % 3 + (k % 4 == 0), replace=False)]
        for n, i in enumerate(where[:1 + k % 3]):
            if (n + k) & 1:
                _miscall(l, i, ord("#"))
            else:
                _miscall(r, insert - 1 - i, ord("#"))
        if k % 4 == 0:   # two good calls that disagree
            _miscall(l, where[-1], ord("F"))
    _write(r1, sides[0], True)
    _write(r2, sides[1], False)
    reads = [[(x[1], x[3]) for x in side] for side in sides]
    want = correct_batch(reads[0], reads[1], s)
    cut = trim_batch(want.reads[0], want.reads[1], ROUTE_TRIM)
    fs = FilterSettings(cut_tail_window=4)
    both = filter_batch(cut.reads[0], cut.reads[1], fs)
    paths = {}
    for name, model, nl in (("m1", want.reads[0], True), ("m2", want.reads[1], False),
                            ("f1", both.reads[0], True), ("f2", both.reads[1], False)):
        paths[name] = str(tmp / (name + ".fq"))
        recs = sides[1] if name.endswith("2") else sides[0]
        _write(paths[name], [[rec[0], b, b"+", q] for rec, (b, q) in zip(recs, model)], nl)
    assert all(t > 0 for t in want.totals), want.totals          # every total is reached
    fusion = [k for k in range(len(sides[0])) if k % 3 != 2]
    assert sum(want.fixed[k] > 0 for k in fusion) > 10 and sum(want.fixed[len(sides[0]) + k] > 0 for k in fusion) > 10
    return dict(paths, fa=fa, lst=lst, csvs=csvs, r1=r1, r2=r2, fs=fs, counters=want.counters(),
                trim_counters=dict(zip(TRIM_KEYS, cut.totals[1:])), filter_counters=both.counters())


def _texts(results):
    from genefuserust_amd import report_json, report_text
    return report_text(results), report_json(results, "cmd", "0.8.0", "t")


def _same_scan(got, want, f, composed=False):
    """(matches or results, counters) of a corrected scan against the plain scan of the model's files.  ``composed``:
    with the trimming and the read filter behind the correction — then ``chunks`` is left out: the model's files hold
    the trimmed reads, so they are shorter texts and take fewer chunks of the same size."""
    (g, g_counters), (w, w_counters) = got, want
    new = NEW_KEYS + ((TRIM_KEYS + RF_KEYS) if composed else ())
    skip = new + (("chunks",) if composed else ())
    assert g == w
    assert {k: v for k, v in g_counters.items() if k not in skip} == \
        {k: v for k, v in w_counters.items() if k not in skip}
    assert ("chunks" in g_counters) == ("chunks" in w_counters)
    assert {k: g_counters[k] for k in NEW_KEYS} == f["counters"]
    keys = list(g_counters)
    at = keys.index(NEW_KEYS[0])
    assert tuple(keys[at:at + len(new)]) == new and keys[at + len(new)] == "complexity"   # in front of the filter counts
    if composed:
        assert {k: g_counters[k] for k in TRIM_KEYS} == f["trim_counters"]
        assert {k: g_counters[k] for k in RF_KEYS} == f["filter_counters"]
    return g_counters


def _steps(f):
    from genefuserust_amd.adapter_trim import AdapterTrim
    from genefuserust_amd.read_filter import ReadFilter
    return dict(adapter_trim=AdapterTrim(adapter_r1=TRUSEQ_R1.decode(), adapter_r2=TRUSEQ_R2.decode()),
                read_filter=ReadFilter(*f["fs"]))


@pytest.mark.gpu
def test_pair_routes(gpu_device, corrected_files):
    from genefuserust_amd.scan import scan_pair_end_files, scan_pair_end_report
    f, cfg = corrected_files, _config(ROUTE_SETTINGS)
    csv = f["csvs"][3]
    files, model, filtered = (f["fa"], csv, f["r1"], f["r2"]), (f["fa"], csv, f["m1"], f["m2"]), \
        (f["fa"], csv, f["f1"], f["f2"])
    want = scan_pair_end_files(*model)
    plain = scan_pair_end_files(*files)
    # (a condition on the fixture, on the model alone: the correction changes what the scan finds)
    assert want[0] != plain[0] and len(want[0]) > 0
    got = scan_pair_end_files(*files, overlap_correct=cfg)
    whole = _same_scan(got, want, f)
    w_results = scan_pair_end_report(*model)
    results = scan_pair_end_report(*files, overlap_correct=cfg)
    _same_scan(results, w_results, f)
    assert _texts(results[0]) == _texts(w_results[0]) and results[1]["fusions"] >= 1
    streamed = scan_pair_end_files(*files, overlap_correct=cfg, chunk_bytes=CHUNK)
    counters = _same_scan(streamed, scan_pair_end_files(*model, chunk_bytes=CHUNK), f)
    assert counters["chunks"] >= 3 and {k: v for k, v in counters.items() if k != "chunks"} == whole
    results = scan_pair_end_report(*files, overlap_correct=cfg, chunk_bytes=CHUNK)
    w_results = scan_pair_end_report(*model, chunk_bytes=CHUNK)
    _same_scan(results, w_results, f)
    assert _texts(results[0]) == _texts(w_results[0])
    # with the trimming and the read filter behind it: the three models in that order, in front of the plain scan
    for kwargs in ({}, dict(chunk_bytes=CHUNK)):
        both = scan_pair_end_files(*files, overlap_correct=cfg, **_steps(f), **kwargs)
        _same_scan(both, scan_pair_end_files(*filtered, **kwargs), f, composed=True)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_bytes", [None, CHUNK])
def test_multi_csv_routes(gpu_device, corrected_files, chunk_bytes):
    from genefuserust_amd.multi_csv_scan import scan_multi_csv_report, scan_report
    f, cfg = corrected_files, _config(ROUTE_SETTINGS)
    got = scan_multi_csv_report(f["fa"], f["lst"], f["r1"], f["r2"], chunk_bytes=chunk_bytes, overlap_correct=cfg)
    want = scan_multi_csv_report(f["fa"], f["lst"], f["m1"], f["m2"], chunk_bytes=chunk_bytes)
    assert [g[0] for g in got] == f["csvs"]
    for (_, results, counters), (_, w_results, w_counters) in zip(got, want):
        _same_scan((results, counters), (w_results, w_counters), f)   # the same totals for every CSV
        assert _texts(results) == _texts(w_results)
    assert sum(1 for g in got if g[2]["fusions"] >= 1) >= 2
    both = scan_multi_csv_report(f["fa"], f["lst"], f["r1"], f["r2"], chunk_bytes=chunk_bytes, overlap_correct=cfg,
                                 **_steps(f))
    w_both = scan_multi_csv_report(f["fa"], f["lst"], f["f1"], f["f2"], chunk_bytes=chunk_bytes)
    for (_, results, counters), (_, w_results, w_counters) in zip(both, w_both):
        _same_scan((results, counters), (w_results, w_counters), f, composed=True)
        assert _texts(results) == _texts(w_results)
    if chunk_bytes is None:   # the mode switch hands the keyword on, to one CSV and to a list
        multi = scan_report(f["fa"], f["lst"], f["r1"], f["r2"], overlap_correct=cfg)
        assert [(c, r, k) for c, r, k in multi] == [(c, r, k) for c, r, k in got]
        one = scan_report(f["fa"], f["csvs"][3], f["r1"], f["r2"], overlap_correct=cfg)
        assert (one[0], one[1]) == (got[3][1], got[3][2])


# ---- what it is for ---------------------------------------------------------------------------------------------------

def _gene(fa: str) -> bytes:
    gene = b"".join(open(fa, "rb").read().split(b"\n")[1:2])[1000:7000]   # GA of the test index
    assert len(gene) == 6000
    return gene


@functools.lru_cache(maxsize=None)
def _miscalled_pairs(gene: bytes):
    """200 pairs of 150-base reads over fragments of 200 bases cut from ``gene`` — an overlap of 100 — with three
    miscalls of low quality inside the overlap, two in one mate and one in the other."""
    rng = np.random.default_rng(14)
    out = []
    for k in range(200):
        at = int(rng.integers(0, len(gene) - 200))
        frag = gene[at:at + 200]
        l = [b"@m%03d/1" % k, frag[:150], b"+", b"F" * 150]
        r = [b"@m%03d/2" % k, rc(frag)[:150], b"+", b"F" * 150]
        for n, i in enumerate(int(x) for x in rng.choice(np.arange(55, 145), 3, replace=False)):
            if (n + k) % 3 == 0:
                _miscall(l, i, ord("#"))
            else:
                _miscall(r, 199 - i, ord("0"))
        out.append((l, r))
    return tuple(out)


@pytest.mark.gpu
def test_miscalled_pairs_merge(gpu_device, corrected_files, tmp_path):
    from genefuserust_amd.scan import scan_pair_end_files
    from oracle import indexer_model as M
    f, cfg = corrected_files, _config(ROUTE_SETTINGS)
    pairs = _miscalled_pairs(_gene(f["fa"]))
    # on the host first: fast_merge merges none of the pairs as they are, and every one once the model has corrected it
    want = correct_batch([(l[1], l[3]) for l, _ in pairs], [(r[1], r[3]) for _, r in pairs], ROUTE_SETTINGS)
    assert want.totals == [200, 200, 200, 400, 600, 0] and want.insert == [200] * 200
    assert sum(M.fast_merge(l[1].decode(), l[3].decode(), r[1].decode(), r[3].decode()) is not None
               for l, r in pairs) == 0
    assert sum(M.fast_merge(a.decode(), qa.decode(), b.decode(), qb.decode()) is not None
               for (a, qa), (b, qb) in zip(*want.reads)) == 200
    r1, r2 = str(tmp_path / "C1.fq"), str(tmp_path / "C2.fq")
    _write(r1, [l for l, _ in pairs], True)
    _write(r2, [r for _, r in pairs], True)
    _, plain = scan_pair_end_files(f["fa"], f["csvs"][3], r1, r2)
    _, fixed = scan_pair_end_files(f["fa"], f["csvs"][3], r1, r2, overlap_correct=cfg)
    assert fixed["pairs"] == 200 and fixed["merged_pairs"] == 200 > plain["merged_pairs"]
    assert {k: fixed[k] for k in NEW_KEYS} == want.counters()
    _, streamed = scan_pair_end_files(f["fa"], f["csvs"][3], r1, r2, overlap_correct=cfg, chunk_bytes=CHUNK)
    assert streamed["merged_pairs"] == 200 and {k: streamed[k] for k in NEW_KEYS} == want.counters()


@pytest.mark.gpu
def test_pcr_copies_with_a_miscall_are_duplicates(gpu_device, corrected_files, tmp_path):
    """60 fragments, three copies each: one clean, one with a low-quality miscall in R1's part of the overlap, one with
    such a miscall in R2's.  The removal keys on the exact bases: it sees 120 duplicates behind the correction, and
    none without it."""
    from genefuserust_amd.dedup import Dedup
    from genefuserust_amd.scan import scan_pair_end_files
    f, cfg = corrected_files, _config(ROUTE_SETTINGS)
    gene, rng = _gene(f["fa"]), np.random.default_rng(15)
    ls, rs = [], []
    for k in range(60):
        frag = gene[97 * k:97 * k + 210]
        for copy in range(3):
            l = [b"@d%03d.%d/1" % (k, copy), frag[:150], b"+", b"F" * 150]
            r = [b"@d%03d.%d/2" % (k, copy), rc(frag)[:150], b"+", b"F" * 150]
            i = int(rng.integers(65, 145))
            if copy == 1:
                _miscall(l, i, ord("#"))
            elif copy == 2:
                _miscall(r, 209 - i, ord("#"))
            ls.append(l)
            rs.append(r)
    want = correct_batch([(l[1], l[3]) for l in ls], [(r[1], r[3]) for r in rs], ROUTE_SETTINGS)
    assert want.totals == [180, 180, 120, 120, 120, 0]
    assert len({(a, b) for (a, _), (b, _) in zip(*want.reads)}) == 60 and len({(l[1], r[1]) for l, r in zip(ls, rs)}) == 180
    r1, r2 = str(tmp_path / "D1.fq"), str(tmp_path / "D2.fq")
    _write(r1, ls, True)
    _write(r2, rs, True)
    for kwargs in ({}, dict(chunk_bytes=CHUNK)):
        _, plain = scan_pair_end_files(f["fa"], f["csvs"][3], r1, r2, dedup=Dedup(), **kwargs)
        _, fixed = scan_pair_end_files(f["fa"], f["csvs"][3], r1, r2, dedup=Dedup(), overlap_correct=cfg, **kwargs)
        assert plain["dedup_duplicates"] == 0 and fixed["dedup_duplicates"] == 120
        assert fixed["corrected_bases"] == 120 and fixed["dedup_unique"] == 60
