"""libgfprep.so on the device (include/gf_read_filter.h): the kernels against the model of the predicate
(tests/read_filter_model.py) — bytes, offsets, reasons and totals, all exact — and every file-level route with
``read_filter`` set against the model in front of the unfiltered scan: the model's output written as FASTQ files, dropped
reads as records with empty sequence and quality lines, scanned with no filter.

Offsets that do not start at 0 are handled as the scans handle them: record i is bytes off[i] .. off[i + 1] of the
input, wherever off[0] lies; the output's offsets start at 0."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.read_filter_cases import GOOD, SETTINGS, bases_of, edge_reads, random_reads
from tests.read_filter_model import KEPT, LOW_QUALITY, MATE_FAILED, TOO_MANY_N, TOO_SHORT, Settings, decide, filter_batch
from tests.test_multi_csv_scan import _files

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_KEYS = ("reads_passed", "reads_trimmed", "bases_trimmed", "reads_too_short", "reads_too_many_n",
            "reads_low_quality", "reads_mate_failed")


@pytest.fixture(scope="module")
def ix(gpu_device):
    from genefuserust_amd import Indexer
    index = Indexer.from_gene_slices([b"ACGT" * 64])
    index.make_index()
    yield index
    index.close()


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


def _held_to_the_model(ix, s: Settings, left, right=None, lead=(0, 0)):
    """One call over the records; everything it leaves equals the model's, byte for byte.  Returns the model's answer."""
    from genefuserust_amd.read_filter import ReadFilter, filter_reads_device
    mates = [] if right is None else [_batch(right, lead[1])]
    *batches, totals, why = filter_reads_device(ix, ReadFilter(*s), _batch(left, lead[0]), *mates, reasons=True)
    want = filter_batch(left, right, s)
    assert len(batches) == len(want.reads)
    for b, reads in zip(batches, want.reads):
        off = b.offsets.cpu().numpy()
        want_off = np.concatenate([[0], np.cumsum([len(r[0]) for r in reads], dtype=np.int64)])
        assert off.shape == want_off.shape and np.array_equal(off, want_off)
        assert b.n_records == len(reads) and b.qual_off is None
        assert b.bases[:int(off[-1])].cpu().numpy().tobytes() == b"".join(r[0] for r in reads)
        assert b.quals[:int(off[-1])].cpu().numpy().tobytes() == b"".join(r[1] for r in reads)
    assert why.cpu().numpy().tolist() == [r for side in want.reasons for r in side]
    assert totals.cpu().numpy().tolist() == want.totals
    return want


@functools.lru_cache(maxsize=None)
def _reads(name: str):
    return tuple(edge_reads(SETTINGS[name]) + random_reads(150, 40))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SETTINGS))
def test_kernel_against_the_model_single_end(ix, name):
    want = _held_to_the_model(ix, SETTINGS[name], list(_reads(name)))
    if name in ("defaults", "window 4"):
        assert set(want.reasons[0]) == {KEPT, TOO_SHORT, TOO_MANY_N, LOW_QUALITY} and want.totals[2] > 10


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["defaults", "window 4", "window 64", "no poly-G"])
def test_kernel_against_the_model_paired(ix, name):
    left = list(_reads(name))
    right = left[37:] + left[:37]          # every record next to another one, at another alignment
    want = _held_to_the_model(ix, SETTINGS[name], left, right, lead=(3, 9))
    assert want.totals[7] > 0 and MATE_FAILED in want.reasons[0] and MATE_FAILED in want.reasons[1]


@pytest.mark.gpu
def test_every_pair_of_verdicts(ix):
    """(kept, each reason) x (kept, each reason): both mates of a pair are dropped when either has a reason."""
    rng = np.random.default_rng(5)
    s = Settings()
    of = {KEPT: (bases_of(rng, 50), bytes([GOOD]) * 50), TOO_SHORT: (bases_of(rng, 9), bytes([GOOD]) * 9),
          TOO_MANY_N: (bases_of(rng, 30) + b"N" * 6 + b"ACA", bytes([GOOD]) * 39),
          LOW_QUALITY: (bases_of(rng, 50), b"#" * 50)}
    assert all(decide(*read, s)[1] == reason for reason, read in of.items())
    combos = [(a, b) for a in of for b in of]
    want = _held_to_the_model(ix, s, [of[a] for a, _ in combos], [of[b] for _, b in combos])
    for k, (a, b) in enumerate(combos):
        assert want.reasons[0][k] == (a or (MATE_FAILED if b else KEPT))
        assert want.reasons[1][k] == (b or (MATE_FAILED if a else KEPT))
    assert want.totals[:2] == [32, 2] and want.totals[4:] == [8, 8, 8, 6]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_batch_sizes(ix, n):
    reads = random_reads(2 * n, 100 + n)
    _held_to_the_model(ix, SETTINGS["window 4"], reads[:n])
    _held_to_the_model(ix, SETTINGS["defaults"], reads[:n], reads[n:], lead=(5, 0))


def _scan_constants():
    src = open(os.path.join(ROOT, "genefuserust_amd", "scan_csrc", "gf_scan_common.h")).read()
    return tuple(int(re.search(r"#define %s (\d+)" % k, src).group(1)) for k in ("GF_SCAN_THREADS", "GF_SCAN_TOTALS_THREADS"))


@pytest.mark.gpu
def test_one_record_past_a_tile_per_thread_of_the_totals_scan(ix):
    threads, totals_threads = _scan_constants()
    n = threads * totals_threads + 1
    rng = np.random.default_rng(8)
    lens = rng.integers(0, 9, n)
    text = rng.choice(np.frombuffer(b"ACGTGGN", dtype=np.uint8), int(lens.sum())).tobytes()
    quals = rng.choice(np.array([35, 60, 73], dtype=np.uint8), int(lens.sum())).tobytes()
    ends = np.cumsum(lens).tolist()
    reads = [(text[e - k:e], quals[e - k:e]) for e, k in zip(ends, lens.tolist())]
    s = Settings(poly_g_min=2, cut_tail_window=2, cut_tail_mean=20, length_required=3, n_base_limit=1,
                 qualified_phred=15, unqualified_percent=50)
    want = _held_to_the_model(ix, s, reads)
    assert want.totals[0] == n and all(t > 1000 for t in want.totals[1:7])


@pytest.mark.gpu
def test_all_dropped_none_touched_and_none_at_all(ix):
    import torch
    from genefuserust_amd.read_filter import ReadFilter, filter_reads_device
    rng = np.random.default_rng(9)
    reads = [(bases_of(rng, L), bytes([GOOD]) * L) for L in rng.integers(20, 200, 700).tolist()]
    want = _held_to_the_model(ix, Settings(length_required=400), reads, reads[::-1])
    assert want.totals == [1400, 0, 0, 0, 1400, 0, 0, 0]
    want = _held_to_the_model(ix, Settings(), reads, reads[::-1], lead=(7, 11))
    assert want.totals == [1400, 1400, 0, 0, 0, 0, 0, 0]
    # none touched: the output is the input, and a lead in front of the first record does not show
    given = _batch(reads, 7)
    kept, _ = filter_reads_device(ix, ReadFilter(), given)
    assert torch.equal(kept.offsets, given.offsets - 7)
    assert torch.equal(kept.bases[:int(kept.offsets[-1])], given.bases[7:]) and torch.equal(
        kept.quals[:int(kept.offsets[-1])], given.quals[7:])
    # no record, and records without a base
    for empty in ([], [(b"", b"")] * 3):
        want = _held_to_the_model(ix, Settings(), empty, empty)
        assert want.totals[0] == 2 * len(empty)


# ---- every route ------------------------------------------------------------------------------------------------------

CHUNKS = (4096, 12_000)


def _records(path):
    lines = open(path, "rb").read().split(b"\n")
    return [lines[k:k + 4] for k in range(0, len(lines) - 3, 4)]


def _write(path, records, final_newline):
    open(path, "wb").write(b"\n".join(b"\n".join(r) for r in records) + (b"\n" if final_newline else b""))


@pytest.fixture(scope="module")
def filtered_files(tmp_path_factory):
    return _filtered_files(tmp_path_factory.mktemp("read_filter_routes"))


def _filtered_files(tmp):
    """tests.test_multi_csv_scan._files with tails and qualities rewritten, so that every reason and both trims occur
    among the pairs that carry a fusion (k % 3 != 2); beside them the model's output as files (F1.fq / F2.fq)."""
    from tests.bgzf_members import bgzf
    fa, lst, csvs, r1, r2 = _files(tmp)
    s = Settings(cut_tail_window=4)
    sides = [_records(r1), _records(r2)]
    for k in range(len(sides[0])):
        kind, (l, r) = k % 10, (sides[0][k], sides[1][k])
        if kind == 0:      # a poly-G tail on R1
            l[1] = l[1][:-25] + b"G" * 25
        elif kind == 1:    # a tail of low quality on R2
            r[3] = r[3][:-40] + b"#" * 40
        elif kind == 3:    # R1 with every other base low: its windows reach the mean, half of its bases are low
            l[3] = (b"I#" * len(l[3]))[:len(l[3])]
        elif kind == 4:    # R2 with eight N
            r[1] = r[1][:60] + b"N" * 8 + r[1][68:]
        elif kind == 6:    # R1 too short
            l[1], l[3] = l[1][:10], l[3][:10]
        elif kind == 7:    # R1 with eight N
            l[1] = l[1][:20] + b"N" * 8 + l[1][28:]
        elif kind == 8:    # a short tail of low quality on R1: what it matched, it still matches, on fewer bases
            l[3] = l[3][:-15] + b"#" * 15
    _write(r1, sides[0], True)
    _write(r2, sides[1], False)
    want = filter_batch([(x[1], x[3]) for x in sides[0]], [(x[1], x[3]) for x in sides[1]], s)
    f1, f2 = str(tmp / "F1.fq"), str(tmp / "F2.fq")
    for path, recs, kept, nl in ((f1, sides[0], want.reads[0], True), (f2, sides[1], want.reads[1], False)):
        _write(path, [[rec[0], b, b"+", q] for rec, (b, q) in zip(recs, kept)], nl)
    single = filter_batch([(x[1], x[3]) for x in sides[0]], None, s)
    f1_single = str(tmp / "F1_single.fq")
    _write(f1_single, [[rec[0], b, b"+", q] for rec, (b, q) in zip(sides[0], single.reads[0])], True)
    fusion = [k for k in range(len(sides[0])) if k % 3 != 2]
    for model in (want, single):
        assert {model.reasons[0][k] for k in fusion} >= {KEPT, TOO_SHORT, TOO_MANY_N, LOW_QUALITY}
        assert all(x > 0 for x in model.totals[1:7])
    assert {want.reasons[1][k] for k in fusion} >= {KEPT, TOO_MANY_N, MATE_FAILED}
    z1, z2 = str(tmp / "Z1.fq.gz"), str(tmp / "Z2.fq.gz")
    for src, dst in ((r1, z1), (r2, z2)):
        open(dst, "wb").write(bgzf(open(src, "rb").read(), sizes=(5000, 777)))
    return dict(fa=fa, lst=lst, csvs=csvs, r1=r1, r2=r2, f1=f1, f2=f2, f1_single=f1_single, z1=z1, z2=z2, s=s,
                pair_counters=want.counters(), single_counters=single.counters(),
                records=[{x[0]: tuple(x) for x in side} for side in sides])


def _config(files):
    from genefuserust_amd.read_filter import ReadFilter
    return ReadFilter(*files["s"])


def _texts(results):
    from genefuserust_amd import report_json, report_text
    return report_text(results), report_json(results, "cmd", "0.8.0", "t")


def _same_scan(got, want, model_counters):
    """(matches or results, counters) of a filtered scan against the unfiltered scan of the model's files.  ``chunks``
    is left out: the model's files hold the trimmed reads, so they are shorter texts and take fewer chunks of the same
    size (the streamed tests hold it to the unfiltered scan of the files themselves instead)."""
    (g, g_counters), (w, w_counters) = got, want
    assert g == w
    assert {k: v for k, v in g_counters.items() if k not in NEW_KEYS + ("chunks",)} == \
        {k: v for k, v in w_counters.items() if k != "chunks"}
    assert ("chunks" in g_counters) == ("chunks" in w_counters)
    assert {k: g_counters[k] for k in NEW_KEYS} == model_counters
    keys = list(g_counters)
    at = keys.index(NEW_KEYS[0])
    assert tuple(keys[at:at + 7]) == NEW_KEYS and keys[at + 7] == "complexity"   # in front of the filter counts
    return g_counters


def _changes_the_outcome(plain, filtered):
    """Matches of the unfiltered scan are gone, and matches are found on a shorter read: otherwise the comparisons
    against the model's files prove nothing."""
    record = lambda m: m.m_name.split(b" ")[0]   # noqa: E731  (without a merged read's suffix)
    shortest = {}
    for m in filtered:
        shortest[record(m)] = min(len(m.m_read), shortest.get(record(m), 1 << 30))
    assert any(record(m) not in shortest for m in plain)
    assert any(shortest.get(record(m), 1 << 30) < len(m.m_read) for m in plain)


@pytest.mark.gpu
def test_pair_routes(gpu_device, filtered_files):
    from genefuserust_amd.scan import scan_pair_end_files, scan_pair_end_report
    f, cfg = filtered_files, _config(filtered_files)
    csv = f["csvs"][3]
    files, model = (f["fa"], csv, f["r1"], f["r2"]), (f["fa"], csv, f["f1"], f["f2"])
    want = scan_pair_end_files(*model)
    plain = scan_pair_end_files(*files)
    got = scan_pair_end_files(*files, read_filter=cfg)
    whole = _same_scan(got, want, f["pair_counters"])
    # the filter changes the outcome: matches are gone, and matches are shorter
    _changes_the_outcome(plain[0], got[0])
    w_results = scan_pair_end_report(*model)
    results = scan_pair_end_report(*files, read_filter=cfg)
    _same_scan(results, w_results, f["pair_counters"])
    assert _texts(results[0]) == _texts(w_results[0]) and results[1]["fusions"] >= 1
    for chunk in CHUNKS:
        streamed = scan_pair_end_files(*files, read_filter=cfg, chunk_bytes=chunk)
        counters = _same_scan(streamed, scan_pair_end_files(*model, chunk_bytes=chunk), f["pair_counters"])
        assert counters["chunks"] >= 3 and {k: v for k, v in counters.items() if k != "chunks"} == whole
        assert counters["chunks"] == scan_pair_end_files(*files, chunk_bytes=chunk)[1]["chunks"]   # the same text
    # originals: the records as the sequencer wrote them, whole file and streamed
    for kwargs in ({}, dict(chunk_bytes=CHUNKS[1])):
        kept, counters = scan_pair_end_files(*files, read_filter=cfg, originals=True, **kwargs)
        assert kept == got[0] and len(kept) > 0
        for m in kept:
            key = m.m_name.split(b" ")[0][:-2]
            assert m.m_original_reads == [f["records"][0][key + b"/1"], f["records"][1][key + b"/2"]]
    # a BGZF copy, inflated on the device
    zipped = scan_pair_end_files(f["fa"], csv, f["z1"], f["z2"], read_filter=cfg, chunk_bytes=CHUNKS[1], inflate="auto")
    assert zipped[0] == got[0] and {k: zipped[1][k] for k in NEW_KEYS} == f["pair_counters"]


@pytest.mark.gpu
def test_single_end_routes(gpu_device, filtered_files):
    from genefuserust_amd.scan import scan_single_end_files, scan_single_end_report
    f, cfg = filtered_files, _config(filtered_files)
    csv = f["csvs"][3]
    files, model = (f["fa"], csv, f["r1"]), (f["fa"], csv, f["f1_single"])
    want = scan_single_end_files(*model)
    got = scan_single_end_files(*files, read_filter=cfg)
    whole = _same_scan(got, want, f["single_counters"])
    plain = scan_single_end_files(*files)
    _changes_the_outcome(plain[0], got[0])
    host = scan_single_end_files(*files, read_filter=cfg, route="host")
    _same_scan(host, scan_single_end_files(*model, route="host"), f["single_counters"])
    assert host[0] == got[0]
    for chunk in CHUNKS:
        streamed = scan_single_end_files(*files, read_filter=cfg, chunk_bytes=chunk)
        counters = _same_scan(streamed, scan_single_end_files(*model, chunk_bytes=chunk), f["single_counters"])
        assert counters["chunks"] >= 3 and {k: v for k, v in counters.items() if k != "chunks"} == whole
        assert counters["chunks"] == scan_single_end_files(*files, chunk_bytes=chunk)[1]["chunks"]
    results, w_results = scan_single_end_report(*files, read_filter=cfg), scan_single_end_report(*model)
    _same_scan(results, w_results, f["single_counters"])
    assert _texts(results[0]) == _texts(w_results[0])
    kept, _ = scan_single_end_files(*files, read_filter=cfg, originals=True, chunk_bytes=CHUNKS[0])
    assert kept == got[0] and all(m.m_original_reads == [f["records"][0][m.m_name]] for m in kept)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_bytes", [None, CHUNKS[1]])
def test_multi_csv_routes(gpu_device, filtered_files, chunk_bytes):
    from genefuserust_amd.multi_csv_scan import scan_multi_csv_report, scan_report
    f, cfg = filtered_files, _config(filtered_files)
    got = scan_multi_csv_report(f["fa"], f["lst"], f["r1"], f["r2"], chunk_bytes=chunk_bytes, read_filter=cfg)
    want = scan_multi_csv_report(f["fa"], f["lst"], f["f1"], f["f2"], chunk_bytes=chunk_bytes)
    assert [g[0] for g in got] == f["csvs"]
    for (_, results, counters), (_, w_results, w_counters) in zip(got, want):
        _same_scan((results, counters), (w_results, w_counters), f["pair_counters"])   # the same totals for every CSV
        assert _texts(results) == _texts(w_results)
    assert sum(1 for g in got if g[2]["fusions"] >= 1) >= 2
    se = scan_multi_csv_report(f["fa"], f["lst"], f["r1"], chunk_bytes=chunk_bytes, read_filter=cfg)
    w_se = scan_multi_csv_report(f["fa"], f["lst"], f["f1_single"], chunk_bytes=chunk_bytes)
    for (_, results, counters), (_, w_results, w_counters) in zip(se, w_se):
        _same_scan((results, counters), (w_results, w_counters), f["single_counters"])
    if chunk_bytes is None:   # the mode switch hands the filter on, to one CSV and to a list
        multi = scan_report(f["fa"], f["lst"], f["r1"], f["r2"], read_filter=cfg)
        assert [(c, r, k) for c, r, k in multi] == [(c, r, k) for c, r, k in got]
        one = scan_report(f["fa"], f["csvs"][3], f["r1"], f["r2"], read_filter=cfg)
        assert (one[0], one[1]) == (got[3][1], got[3][2])


@pytest.mark.gpu
def test_the_command_line_in_a_child_process(gpu_device, filtered_files, tmp_path):
    from genefuserust_amd.scan import scan_pair_end_report
    f, cfg = filtered_files, _config(filtered_files)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "genefuserust_amd", "-1", f["r1"], "-2", f["r2"], "-f", f["csvs"][3], "-r",
                          f["fa"], "-h", "", "-j", "out.json", "--read-filter", "--cut-tail-window", "4"],
                         cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    results, counters = scan_pair_end_report(f["fa"], f["csvs"][3], f["r1"], f["r2"], read_filter=cfg)
    plain, _ = scan_pair_end_report(f["fa"], f["csvs"][3], f["r1"], f["r2"])
    assert counters["fusions"] >= 1 and _texts(results)[0] != _texts(plain)[0]
    assert _texts(results)[0] in run.stdout and _texts(plain)[0] not in run.stdout
    body = lambda text: text[text.index('"fusions"'):]   # noqa: E731  (behind the command, the version and the time)
    assert body(open(str(tmp_path / "out.json")).read()) == body(_texts(results)[1])
