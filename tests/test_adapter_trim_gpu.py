"""libgfadapt.so on the device (include/gf_adapter_trim.h): the kernels against the model of the predicate
(tests/adapter_trim_model.py) — bytes, offsets, codes and totals, all exact — every file-level route with
``adapter_trim`` set against the model in front of the plain scan (the model's output written as FASTQ files and scanned
without the keyword), and what the trimming is for: read-through pairs merge.

Offsets that do not start at 0 are handled as the scans handle them: record i is bytes off[i] .. off[i + 1] of the
input, wherever off[0] lies; the output's offsets start at 0."""
import functools
import os

import numpy as np
import pytest

from tests.adapter_trim_cases import (SETTINGS, bases_of, modelled, pair_cases, quals_of, rc, read_through,
                                      single_cases)
from tests.adapter_trim_model import (BY_OVERLAP, BY_SEQUENCE, OVERLAP_CLEAN, TOTAL_KEYS, TRUSEQ_R1, TRUSEQ_R2,
                                      UNTOUCHED, Settings, trim_batch)
from tests.test_multi_csv_scan import _files

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_KEYS = TOTAL_KEYS[1:]
RF_KEYS = ("reads_passed", "reads_trimmed", "bases_trimmed", "reads_too_short", "reads_too_many_n",
           "reads_low_quality", "reads_mate_failed")


@pytest.fixture(scope="module")
def ix(gpu_device):
    from genefuserust_amd import Indexer
    index = Indexer.from_gene_slices([b"ACGT" * 64])
    index.make_index()
    yield index
    index.close()


def _config(s: Settings):
    from genefuserust_amd.adapter_trim import AdapterTrim
    return AdapterTrim(bool(s.overlap), s.adapter_r1.decode(), s.adapter_r2.decode(), s.min_overlap, s.max_diff,
                       s.diff_percent, s.min_adapter)


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


def _held_to_the_model(ix, s: Settings, left, right, verdicts, lead=(0, 0)):
    """One call over the records (bases only: the qualities are ``quals_of``); everything it leaves equals the model's,
    byte for byte.  ``verdicts``: the model's, record by record.  Returns the model's answer."""
    from genefuserust_amd.adapter_trim import trim_adapters_device
    with_q = lambda side: [(x, quals_of(x)) for x in side]   # noqa: E731
    left, right = with_q(left), None if right is None else with_q(right)
    mates = [] if right is None else [_batch(right, lead[1])]
    *batches, totals, how = trim_adapters_device(ix, _config(s), _batch(left, lead[0]), *mates, how=True)
    want = trim_batch(left, right, s, verdicts)
    assert len(batches) == len(want.reads)
    for b, reads in zip(batches, want.reads):
        off = b.offsets.cpu().numpy()
        want_off = np.concatenate([[0], np.cumsum([len(r[0]) for r in reads], dtype=np.int64)])
        assert off.shape == want_off.shape and np.array_equal(off, want_off)
        assert b.n_records == len(reads) and b.qual_off is None
        assert b.bases[:int(off[-1])].cpu().numpy().tobytes() == b"".join(r[0] for r in reads)
        assert b.quals[:int(off[-1])].cpu().numpy().tobytes() == b"".join(r[1] for r in reads)
    assert how.cpu().numpy().tolist() == [c for side in want.how for c in side]
    assert totals.cpu().numpy().tolist() == want.totals
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SETTINGS))
def test_kernel_against_the_model_paired(ix, name):
    """Two tiles; the two sides at different alignments."""
    pairs = pair_cases(name)
    assert len(pairs) > 256
    want = _held_to_the_model(ix, SETTINGS[name], [a for a, _ in pairs], [b for _, b in pairs], modelled(name),
                              lead=(3, 9))
    if name == "illumina":   # every code, and every total
        assert {c for side in want.how for c in side} == {UNTOUCHED, BY_OVERLAP, BY_SEQUENCE, OVERLAP_CLEAN}
        assert all(t > 0 for t in want.totals)
        assert BY_SEQUENCE in want.how[0] and BY_SEQUENCE in want.how[1]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["illumina", "sequence only", "percent 10", "smallest"])
def test_kernel_against_the_model_single_end(ix, name):
    reads = single_cases(name)
    want = _held_to_the_model(ix, SETTINGS[name], list(reads), None, modelled(name, True), lead=(5, 0))
    assert set(want.how[0]) == {UNTOUCHED, BY_SEQUENCE} and want.totals[3] == want.totals[5] == 0
    assert want.totals[1] == want.totals[4] > 10 and want.totals[2] > 100


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 600])
def test_batch_sizes(ix, n):
    """One tile, the tile's edges, and a partial third tile: the cases again and again, each at another place."""
    pairs, verdicts = pair_cases("illumina"), modelled("illumina")
    at = [(7 * n + k) % len(pairs) for k in range(n)]
    _held_to_the_model(ix, SETTINGS["illumina"], [pairs[k][0] for k in at], [pairs[k][1] for k in at],
                       [verdicts[k] for k in at], lead=(3, 9))
    reads, verdicts = single_cases("illumina"), modelled("illumina", True)
    at = [(3 * n + k) % len(reads) for k in range(n)]
    _held_to_the_model(ix, SETTINGS["illumina"], [reads[k] for k in at], None, [verdicts[k] for k in at])


@pytest.mark.gpu
def test_none_touched_and_none_at_all(ix):
    import torch
    from genefuserust_amd.adapter_trim import AdapterTrim, trim_adapters_device
    rng = np.random.default_rng(9)
    reads = [bases_of(rng, L) for L in rng.integers(20, 29, 300).tolist()]   # too short for any candidate
    s = Settings()
    verdicts = [((len(a), UNTOUCHED), (len(b), UNTOUCHED)) for a, b in zip(reads, reads[::-1])]
    want = _held_to_the_model(ix, s, reads, reads[::-1], verdicts, lead=(7, 11))
    assert want.totals == [600, 0, 0, 0, 0, 0]
    given = _batch([(x, quals_of(x)) for x in reads], 7)
    kept, mate, _ = trim_adapters_device(ix, AdapterTrim(), given, given)
    assert torch.equal(kept.offsets, given.offsets - 7) and torch.equal(mate.offsets, kept.offsets)
    assert torch.equal(kept.bases[:int(kept.offsets[-1])], given.bases[7:]) and torch.equal(
        kept.quals[:int(kept.offsets[-1])], given.quals[7:])
    # no record, and records without a base
    for empty in ([], [b""] * 3):
        want = _held_to_the_model(ix, s, empty, empty, [((0, UNTOUCHED), (0, UNTOUCHED))] * len(empty))
        assert want.totals == [2 * len(empty), 0, 0, 0, 0, 0]


# ---- every route ------------------------------------------------------------------------------------------------------

CHUNK = 12_000
ROUTE_SETTINGS = Settings(adapter_r1=TRUSEQ_R1, adapter_r2=TRUSEQ_R2)


def _records(path):
    lines = open(path, "rb").read().split(b"\n")
    return [lines[k:k + 4] for k in range(0, len(lines) - 3, 4)]


def _write(path, records, final_newline):
    open(path, "wb").write(b"\n".join(b"\n".join(r) for r in records) + (b"\n" if final_newline else b""))


@pytest.fixture(scope="module")
def trimmed_files(tmp_path_factory):
    return _trimmed_files(tmp_path_factory.mktemp("adapter_trim_routes"))


def _trimmed_files(tmp):
    """tests.test_multi_csv_scan._files with fragments shortened, so that pairs that carry a fusion (k % 3 != 2) read
    through into the adapters, and mates spoiled, so that the sequence step cuts the other; beside them the model's
    output as files (M1.fq / M2.fq, and for single-end input M1_single.fq), and with the read filter's model behind it
    (F1.fq / F2.fq)."""
    from tests.read_filter_model import Settings as FilterSettings
    from tests.read_filter_model import filter_batch
    fa, lst, csvs, r1, r2 = _files(tmp)
    rng = np.random.default_rng(31)
    s = ROUTE_SETTINGS
    sides = [_records(r1), _records(r2)]
    for k in range(len(sides[0])):
        kind, (l, r) = k % 5, (sides[0][k], sides[1][k])
        if kind == 0:      # a fragment of the first 95 to 140 bases of R1, read through by both mates
            a, b = read_through(rng, l[1][:int(rng.integers(95, 141))], 150, 150, s)
            l[1], r[1] = a, b
        elif kind == 1:    # R1 reads through, R2 is spoiled: no insert length, R1 is cut by its adapter
            l[1] = read_through(rng, l[1][:120], 150, 150, s)[0]
            r[1] = b"N" * 60 + r[1][60:]
        elif kind == 3:    # the same for R2
            r[1] = read_through(rng, rc(r[1][:110]), 150, 150, s)[1]
            l[1] = l[1][:40] + b"N" * 70 + l[1][110:]
        for x in (l, r):
            x[3] = (x[3] + b"F" * 150)[:len(x[1])]
    _write(r1, sides[0], True)
    _write(r2, sides[1], False)
    reads = [[(x[1], x[3]) for x in side] for side in sides]
    want = trim_batch(reads[0], reads[1], s)
    single = trim_batch(reads[0], None, s)
    fs = FilterSettings(cut_tail_window=4)
    both = filter_batch(want.reads[0], want.reads[1], fs)
    paths = {}
    for name, model, nl in (("m1", want.reads[0], True), ("m2", want.reads[1], False), ("m1_single", single.reads[0], True),
                            ("f1", both.reads[0], True), ("f2", both.reads[1], False)):
        paths[name] = str(tmp / (name + ".fq"))
        recs = sides[1] if name.endswith("2") else sides[0]
        _write(paths[name], [[rec[0], b, b"+", q] for rec, (b, q) in zip(recs, model)], nl)
    fusion = [k for k in range(len(sides[0])) if k % 3 != 2]
    assert {want.how[0][k] for k in fusion} == {UNTOUCHED, BY_OVERLAP, BY_SEQUENCE, OVERLAP_CLEAN}
    assert BY_SEQUENCE in {want.how[1][k] for k in fusion} and all(t > 0 for t in want.totals)
    assert set(single.how[0]) == {UNTOUCHED, BY_SEQUENCE} and single.totals[4] > 20
    return dict(paths, fa=fa, lst=lst, csvs=csvs, r1=r1, r2=r2, fs=fs, pair_counters=want.counters(),
                single_counters=single.counters(), filter_counters=both.counters())


def _route_config():
    return _config(ROUTE_SETTINGS)


def _texts(results):
    from genefuserust_amd import report_json, report_text
    return report_text(results), report_json(results, "cmd", "0.8.0", "t")


def _same_scan(got, want, model_counters, filter_counters=None):
    """(matches or results, counters) of a trimmed scan against the plain scan of the model's files.  ``chunks`` is left
    out: the model's files hold the trimmed reads, so they are shorter texts and take fewer chunks of the same size."""
    (g, g_counters), (w, w_counters) = got, want
    new = NEW_KEYS + (RF_KEYS if filter_counters is not None else ())
    assert g == w
    assert {k: v for k, v in g_counters.items() if k not in new + ("chunks",)} == \
        {k: v for k, v in w_counters.items() if k != "chunks"}
    assert ("chunks" in g_counters) == ("chunks" in w_counters)
    assert {k: g_counters[k] for k in NEW_KEYS} == model_counters
    keys = list(g_counters)
    at = keys.index(NEW_KEYS[0])
    assert tuple(keys[at:at + len(new)]) == new and keys[at + len(new)] == "complexity"   # in front of the filter counts
    if filter_counters is not None:
        assert {k: g_counters[k] for k in RF_KEYS} == filter_counters
    return g_counters


@pytest.mark.gpu
def test_pair_routes(gpu_device, trimmed_files):
    from genefuserust_amd.read_filter import ReadFilter
    from genefuserust_amd.scan import scan_pair_end_files, scan_pair_end_report
    f, cfg = trimmed_files, _route_config()
    csv = f["csvs"][3]
    files, model = (f["fa"], csv, f["r1"], f["r2"]), (f["fa"], csv, f["m1"], f["m2"])
    want = scan_pair_end_files(*model)
    plain = scan_pair_end_files(*files)
    got = scan_pair_end_files(*files, adapter_trim=cfg)
    whole = _same_scan(got, want, f["pair_counters"])
    # the trimming changes the outcome: pairs merge that did not, and the matches are others
    assert whole["merged_pairs"] > plain[1]["merged_pairs"] and got[0] != plain[0] and len(got[0]) > 0
    w_results = scan_pair_end_report(*model)
    results = scan_pair_end_report(*files, adapter_trim=cfg)
    _same_scan(results, w_results, f["pair_counters"])
    assert _texts(results[0]) == _texts(w_results[0]) and results[1]["fusions"] >= 1
    streamed = scan_pair_end_files(*files, adapter_trim=cfg, chunk_bytes=CHUNK)
    counters = _same_scan(streamed, scan_pair_end_files(*model, chunk_bytes=CHUNK), f["pair_counters"])
    assert counters["chunks"] >= 3 and {k: v for k, v in counters.items() if k != "chunks"} == whole
    assert counters["chunks"] == scan_pair_end_files(*files, chunk_bytes=CHUNK)[1]["chunks"]   # the same text
    # with the read filter behind it: the trimming's model, then the filter's, in front of the plain scan
    rf = ReadFilter(*f["fs"])
    filtered = (f["fa"], csv, f["f1"], f["f2"])
    for kwargs in ({}, dict(chunk_bytes=CHUNK)):
        both = scan_pair_end_files(*files, adapter_trim=cfg, read_filter=rf, **kwargs)
        _same_scan(both, scan_pair_end_files(*filtered, **kwargs), f["pair_counters"], f["filter_counters"])


@pytest.mark.gpu
def test_single_end_routes(gpu_device, trimmed_files):
    from genefuserust_amd.scan import scan_single_end_files, scan_single_end_report
    f, cfg = trimmed_files, _route_config()
    csv = f["csvs"][3]
    files, model = (f["fa"], csv, f["r1"]), (f["fa"], csv, f["m1_single"])
    want = scan_single_end_files(*model)
    got = scan_single_end_files(*files, adapter_trim=cfg)
    whole = _same_scan(got, want, f["single_counters"])
    assert got[0] != scan_single_end_files(*files)[0]
    host = scan_single_end_files(*files, adapter_trim=cfg, route="host")
    _same_scan(host, scan_single_end_files(*model, route="host"), f["single_counters"])
    assert host[0] == got[0]
    streamed = scan_single_end_files(*files, adapter_trim=cfg, chunk_bytes=CHUNK)
    counters = _same_scan(streamed, scan_single_end_files(*model, chunk_bytes=CHUNK), f["single_counters"])
    assert counters["chunks"] >= 3 and {k: v for k, v in counters.items() if k != "chunks"} == whole
    results, w_results = scan_single_end_report(*files, adapter_trim=cfg), scan_single_end_report(*model)
    _same_scan(results, w_results, f["single_counters"])
    assert _texts(results[0]) == _texts(w_results[0])


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_bytes", [None, CHUNK])
def test_multi_csv_routes(gpu_device, trimmed_files, chunk_bytes):
    from genefuserust_amd.multi_csv_scan import scan_multi_csv_report, scan_report
    f, cfg = trimmed_files, _route_config()
    got = scan_multi_csv_report(f["fa"], f["lst"], f["r1"], f["r2"], chunk_bytes=chunk_bytes, adapter_trim=cfg)
    want = scan_multi_csv_report(f["fa"], f["lst"], f["m1"], f["m2"], chunk_bytes=chunk_bytes)
    assert [g[0] for g in got] == f["csvs"]
    for (_, results, counters), (_, w_results, w_counters) in zip(got, want):
        _same_scan((results, counters), (w_results, w_counters), f["pair_counters"])   # the same totals for every CSV
        assert _texts(results) == _texts(w_results)
    assert sum(1 for g in got if g[2]["fusions"] >= 1) >= 2
    se = scan_multi_csv_report(f["fa"], f["lst"], f["r1"], chunk_bytes=chunk_bytes, adapter_trim=cfg)
    w_se = scan_multi_csv_report(f["fa"], f["lst"], f["m1_single"], chunk_bytes=chunk_bytes)
    for (_, results, counters), (_, w_results, w_counters) in zip(se, w_se):
        _same_scan((results, counters), (w_results, w_counters), f["single_counters"])
    if chunk_bytes is None:   # the mode switch hands the keyword on, to one CSV and to a list
        multi = scan_report(f["fa"], f["lst"], f["r1"], f["r2"], adapter_trim=cfg)
        assert [(c, r, k) for c, r, k in multi] == [(c, r, k) for c, r, k in got]
        one = scan_report(f["fa"], f["csvs"][3], f["r1"], f["r2"], adapter_trim=cfg)
        assert (one[0], one[1]) == (got[3][1], got[3][2])


# ---- what it is for ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _read_through_pairs(gene: bytes):
    """200 pairs of 150-base reads over inserts of 100 bases cut from ``gene``: TruSeq adapters, then random bases."""
    rng = np.random.default_rng(12)
    pairs = []
    for _ in range(200):
        at = int(rng.integers(0, len(gene) - 100))
        pairs.append(read_through(rng, gene[at:at + 100], 150, 150, ROUTE_SETTINGS))
    return tuple(pairs)


@pytest.mark.gpu
def test_read_through_pairs_merge(gpu_device, trimmed_files, tmp_path):
    from genefuserust_amd.scan import scan_pair_end_files
    from oracle import indexer_model as M
    f = trimmed_files
    gene = b"".join(open(f["fa"], "rb").read().split(b"\n")[1:2])[1000:7000]   # GA of the test index
    assert len(gene) == 6000
    pairs = _read_through_pairs(gene)
    # on the host first: fast_merge merges none of the pairs as they are, and every one once the model has cut it
    q = "F" * 150
    cut = trim_batch([(a, q.encode()) for a, _ in pairs], [(b, q.encode()) for _, b in pairs], ROUTE_SETTINGS)
    assert cut.totals == [400, 400, 400 * 50, 400, 0, 200]
    assert sum(M.fast_merge(a.decode(), q, b.decode(), q) is not None for a, b in pairs) == 0
    assert sum(M.fast_merge(a.decode(), qa.decode(), b.decode(), qb.decode()) is not None
               for (a, qa), (b, qb) in zip(*cut.reads)) == 200
    r1, r2 = str(tmp_path / "T1.fq"), str(tmp_path / "T2.fq")
    _write(r1, [[b"@t%03d/1" % k, a, b"+", q.encode()] for k, (a, _) in enumerate(pairs)], True)
    _write(r2, [[b"@t%03d/2" % k, b, b"+", q.encode()] for k, (_, b) in enumerate(pairs)], True)
    _, plain = scan_pair_end_files(f["fa"], f["csvs"][3], r1, r2)
    _, trimmed = scan_pair_end_files(f["fa"], f["csvs"][3], r1, r2, adapter_trim=_route_config())
    assert trimmed["pairs"] == 200 and trimmed["merged_pairs"] == 200 > plain["merged_pairs"]
    assert {k: trimmed[k] for k in NEW_KEYS} == cut.counters()
