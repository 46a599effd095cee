"""libgfqc.so on the device (include/gf_read_qc.h): the stats kernel and the insert kernel against the model
(tests/read_qc_model.py) — every table compared with ``array_equal``, never approximately — at the edges of the table's
layout and of the launch, accumulation over calls, and every route of a scan with ``qc``: whole file against streamed,
both against the model over the files, with and without the adapter trimming and the read filter in between."""
import functools
import os
import re

import numpy as np
import pytest

from genefuserust_amd import read_qc
from tests.read_qc_cases import LENGTHS, edge_reads, insert_entries, insert_pairs, short_reads, with_quals
from tests.read_qc_model import INSERT_WORDS, SIDE_WORDS, fastq_records, insert_hist, stats_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# gf_qc_kernels.h: a launch has at most GF_QC_GRID = 768 blocks of 256 threads — 3072 wavefronts of the stats kernel,
# 12288 groups of 16 lanes of the insert kernel; a wavefront (a group) takes every 3072nd record (every 12288th pair)
GRID = 768
WAVES, GROUPS = GRID * 4, GRID * 16


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


def _batch(reads, lead: int = 0):
    """The records as the full FASTQ cut leaves them; ``lead`` bytes of another record in front of the first."""
    off = lead + np.concatenate([[0], np.cumsum([len(r[0]) for r in reads], dtype=np.int64)])
    return _batch_at(b"G" * lead + b"".join(r[0] for r in reads), b"~" * lead + b"".join(r[1] for r in reads), off)


def _table(prefilled=None):
    import torch
    if prefilled is not None:
        return torch.from_numpy(np.asarray(prefilled, dtype=np.int64).copy()).cuda()
    return torch.zeros(SIDE_WORDS, dtype=torch.int64, device="cuda")


def _hist():
    import torch
    return torch.zeros(INSERT_WORDS, dtype=torch.int64, device="cuda")


def _stats(ix, reads, lead=0):
    t = _table()
    read_qc.qc_stats_device(ix, _batch(reads, lead), t)
    return t.cpu().numpy()


def test_the_grid_constant_is_the_one_stated_here():
    kernels = open(os.path.join(ROOT, "genefuserust_amd", "scan_csrc", "gf_qc_kernels.h")).read()
    assert int(re.search(r"#define GF_QC_GRID (\d+)", kernels).group(1)) == GRID
    assert "#define GF_SCAN_THREADS 256" in open(os.path.join(ROOT, "genefuserust_amd", "scan_csrc",
                                                              "gf_scan_common.h")).read()


@pytest.mark.gpu
def test_stats_against_the_model_at_every_edge(ix):
    """Every length of the cases, every byte class and quality threshold, the two sides at different alignments, and
    one record whose offsets run backwards."""
    reads = list(edge_reads())
    assert sorted({len(b) for b, _ in reads}) == LENGTHS
    want = stats_table(reads)
    for lead, side in ((3, reads), (9, reads[::-1])):
        assert np.array_equal(_stats(ix, side, lead), want), lead
    cycles = want[513:].reshape(513, 8)
    assert (cycles[[0, 63, 64, 511, 512], :5].sum(axis=1) > 0).all() and (cycles[512] > 0).all()
    assert want[0] == 2 and want[512] == 10
    # offsets that run backwards: a record of length 0, and the next record starts where they point
    lead, b, q = 5, b"".join(r[0] for r in reads), b"".join(r[1] for r in reads)
    off = [lead + int(x) for x in np.concatenate([[0], np.cumsum([len(r[0]) for r in reads])])]
    j = next(k for k, r in enumerate(reads) if len(r[0]) == 4096)
    off[j + 1:j + 1] = [off[j] + 20, off[j] + 3]
    bb, qq = b"G" * lead + b, b"~" * lead + q
    cut = [(bb[s:max(s, e)], qq[s:max(s, e)]) for s, e in zip(off, off[1:])]
    assert [len(x[0]) for x in cut[j:j + 3]] == [20, 0, 4093] and len(cut) == len(reads) + 2
    t = _table()
    read_qc.qc_stats_device(ix, _batch_at(bb, qq, off), t)
    assert np.array_equal(t.cpu().numpy(), stats_table(cut))


@functools.lru_cache(maxsize=None)
def _mixed():
    return tuple(r for r in edge_reads() if len(r[0]) <= 600) + short_reads(64)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 600])
def test_batch_sizes(ix, n):
    """No record (nothing is queued, the table stays), one, around one block's worth of wavefronts' first records."""
    cases = _mixed()
    reads = [cases[(7 * n + k) % len(cases)] for k in range(n)]
    assert np.array_equal(_stats(ix, reads, lead=n % 16), stats_table(reads))
    pairs, entries = insert_pairs(), insert_entries()
    at = [(5 * n + k) % len(pairs) for k in range(n)]
    h = _hist()
    read_qc.qc_insert_device(ix, _batch(with_quals([pairs[k][0] for k in at]), 3),
                             _batch(with_quals([pairs[k][1] for k in at]), 9), h)
    assert np.array_equal(h.cpu().numpy(), np.bincount([entries[k] for k in at], minlength=INSERT_WORDS))


@pytest.mark.gpu
def test_more_records_than_the_launch_has_wavefronts(ix):
    """2 x 3072 + 57 short reads: every wavefront's loop over its records runs at least twice, 57 of them three times.
    2 x 12288 + 57 short pairs, a few of the cases among them: the same for every group of the insert kernel."""
    n = 2 * WAVES + 57
    reads = short_reads(n)
    want = stats_table(reads)
    assert np.array_equal(_stats(ix, reads, lead=7), want) and want[1:41].sum() == n
    rng = np.random.default_rng(3)
    n = 2 * GROUPS + 57
    left = [bytes(x) for x in np.split(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 20 * n), n)]
    right = [x[:int(L)] for x, L in zip(left[::-1], rng.integers(1, 21, n))]
    entries = [0] * n   # (mates of at most 20 bases have no candidate: L1 + L2 - 30 < 30)
    pairs, known = insert_pairs(), insert_entries()
    for k, at in enumerate(range(11, n, n // 40)):
        left[at], right[at] = pairs[(7 * k) % len(pairs)]
        entries[at] = known[(7 * k) % len(pairs)]
    h = _hist()
    read_qc.qc_insert_device(ix, _batch(with_quals(left), 1), _batch(with_quals(right), 2), h)
    want = np.bincount(entries, minlength=INSERT_WORDS)
    assert np.array_equal(h.cpu().numpy(), want) and (want[30:1025] > 0).sum() >= 5


@pytest.mark.gpu
def test_calls_accumulate_and_a_table_keeps_its_contents(ix):
    first, second = list(edge_reads()[:12]), list(_mixed()[5:60])
    t = _table()
    read_qc.qc_stats_device(ix, _batch(first, 3), t)
    read_qc.qc_stats_device(ix, _batch(second, 9), t)
    assert np.array_equal(t.cpu().numpy(), stats_table(first + second))
    filled = np.arange(SIDE_WORDS, dtype=np.int64) * 3 + (1 << 40)   # (past 32 bits: the words are 64-bit)
    t = _table(filled)
    read_qc.qc_stats_device(ix, _batch(second), t)
    assert np.array_equal(t.cpu().numpy(), filled + stats_table(second))
    read_qc.qc_stats_device(ix, _batch([]), t)   # no record: nothing is added
    assert np.array_equal(t.cpu().numpy(), filled + stats_table(second))
    pairs, entries = insert_pairs(), insert_entries()
    h = _hist()
    for part in (slice(0, 100), slice(100, None)):
        read_qc.qc_insert_device(ix, _batch(with_quals([a for a, _ in pairs[part]])),
                                 _batch(with_quals([b for _, b in pairs[part]])), h)
    assert np.array_equal(h.cpu().numpy(), np.bincount(entries, minlength=INSERT_WORDS))


@pytest.mark.gpu
def test_insert_histogram_against_the_model(ix):
    """The pairs the adapter trimming is held to, and own ones up to the top of the histogram; the two sides at
    different alignments."""
    from tests.adapter_trim_cases import pair_cases
    pairs, entries = insert_pairs(), insert_entries()
    n = len(pair_cases("illumina"))
    illumina = entries[:n]
    measured = [e for e in illumina if 30 <= e <= 1024]
    assert (n, illumina.count(1025), illumina.count(0)) == (289, 13, 159)
    assert len(set(measured)) > 50 and min(measured) == 30 and max(measured) == 512
    assert entries[n:] == (994, 900, 30) and [len(a) for a, _ in pairs[n:n + 2]] == [512, 512]
    h = _hist()
    read_qc.qc_insert_device(ix, _batch(with_quals([a for a, _ in pairs]), 3),
                             _batch(with_quals([b for _, b in pairs]), 9), h)
    got = h.cpu().numpy()
    assert np.array_equal(got, np.bincount(entries, minlength=INSERT_WORDS))
    assert np.array_equal(got, insert_hist(pairs[n:], np.bincount(illumina, minlength=INSERT_WORDS)))
    assert not got[1:30].any() and not got[995:1025].any() and got[994] == 1 and got[1025] == 13


# ---- every route ------------------------------------------------------------------------------------------------------

CHUNK = 12_000


@pytest.fixture(scope="module")
def files(tmp_path_factory, gpu_device):
    """The planted FASTQ pair of tests.test_multi_csv_scan._files with fragments that read through
    (tests.test_adapter_trim_gpu._trimmed_files, which also writes the trimming's and the filter's model output as
    files), and the model's tables over them, computed once."""
    from tests.test_adapter_trim_gpu import _trimmed_files
    tmp = tmp_path_factory.mktemp("read_qc_routes")
    f = _trimmed_files(tmp)
    sides = [fastq_records(f["r1"]), fastq_records(f["r2"])]
    f["before"] = [stats_table(s) for s in sides]
    f["inserts"] = insert_hist([(a[0], b[0]) for a, b in zip(*sides)])
    f["after"] = [stats_table(fastq_records(f[k])) for k in ("f1", "f2")]           # trimmed, then filtered
    f["after_single"] = stats_table(fastq_records(f["m1_single"]))                  # R1 alone, trimmed by sequence
    two = tmp / "two.txt"
    two.write_text("%s\n%s\n" % (f["csvs"][3], f["csvs"][0]))
    f["two"] = str(two)
    return f


def _same_result(got, before, after, inserts):
    assert len(got.before) == len(before) and len(got.after) == len(after)
    for g, w in zip(got.before + got.after, list(before) + list(after)):
        assert g.dtype == np.int64 and np.array_equal(g, w)
    assert (got.insert is None) == (inserts is None)
    if inserts is not None:
        assert np.array_equal(got.insert, inserts)


@pytest.mark.gpu
def test_pair_routes_whole_file_and_streamed(files):
    from genefuserust_amd.read_qc import ReadQc
    from genefuserust_amd.scan import scan_pair_end_files, scan_pair_end_report
    f = files
    args = (f["fa"], f["csvs"][3], f["r1"], f["r2"])
    whole, streamed, report = ReadQc(), ReadQc(), ReadQc(insert_size=False)
    plain = scan_pair_end_files(*args)
    assert scan_pair_end_files(*args, qc=whole) == plain and len(plain[0]) > 0
    plain_streamed = scan_pair_end_files(*args, chunk_bytes=CHUNK)
    assert scan_pair_end_files(*args, chunk_bytes=CHUNK, qc=streamed) == plain_streamed
    assert plain_streamed[1]["chunks"] >= 3   # records straddle chunks, and none is counted twice
    assert scan_pair_end_report(*args, qc=report)[1] == scan_pair_end_report(*args)[1]
    # neither trimming nor filter: "after" is "before", measured once
    _same_result(whole.result(), f["before"], f["before"], f["inserts"])
    _same_result(streamed.result(), f["before"], f["before"], f["inserts"])
    _same_result(report.result(), f["before"], f["before"], None)
    assert f["inserts"][30:1025].sum() >= 20 and f["inserts"][0] > 0   # pairs that read through, and pairs that do not
    assert f["before"][0][150] == 150 and whole.result().summary("before")["total_reads"] == 300


@pytest.mark.gpu
def test_pair_routes_with_trimming_and_filter(files):
    """ "after" is the model's table over the output of ``trim_batch``, then of the read filter's model; a dropped
    record lands in length_hist[0] and in no cycle row."""
    from genefuserust_amd.read_filter import ReadFilter
    from genefuserust_amd.read_qc import ReadQc, report_json
    from genefuserust_amd.scan import scan_pair_end_files
    from tests.test_adapter_trim_gpu import _route_config
    from tests import read_qc_model as model
    f = files
    args = (f["fa"], f["csvs"][3], f["r1"], f["r2"])
    ahead = dict(adapter_trim=_route_config(), read_filter=ReadFilter(*f["fs"]))
    counters = None
    for kwargs in ({}, dict(chunk_bytes=CHUNK)):
        qc = ReadQc()
        got = scan_pair_end_files(*args, **ahead, **kwargs, qc=qc)
        assert got == scan_pair_end_files(*args, **ahead, **kwargs)
        r = qc.result()
        _same_result(r, f["before"], f["after"], f["inserts"])
        counters = got[1]
        assert report_json(r, counters) == model.report_json(f["before"], f["after"], f["inserts"], counters)
    dropped = sum(counters[k] for k in ("reads_too_short", "reads_too_many_n", "reads_low_quality", "reads_mate_failed"))
    assert dropped > 0 and f["after"][0][0] + f["after"][1][0] == dropped
    after = r.summary("after")
    assert after["total_reads"] == counters["reads_passed"] == 300 - dropped
    # every base is accounted for: cut by the trimming, cut off a kept read by the filter, or dropped with its read
    assert after["total_bases"] == r.summary("before")["total_bases"] - counters["adapter_bases_cut"] \
        - counters["bases_trimmed"] - _bases_of_dropped(f)


def _bases_of_dropped(f) -> int:
    """The bases the trimmed reads had that the filter then dropped whole: trimmed minus filtered, less the bases the
    filter cut off kept reads."""
    trimmed = [fastq_records(f[k]) for k in ("m1", "m2")]
    kept = [fastq_records(f[k]) for k in ("f1", "f2")]
    return sum(len(t[0]) for side, after in zip(trimmed, kept) for t, k in zip(side, after) if not k[0])


@pytest.mark.gpu
def test_single_end_routes(files):
    from genefuserust_amd.read_qc import ReadQc
    from genefuserust_amd.scan import scan_single_end_files
    from tests.test_adapter_trim_gpu import _route_config
    f = files
    args = (f["fa"], f["csvs"][3], f["r1"])
    for kwargs in (dict(route="device"), dict(route="host"), dict(chunk_bytes=CHUNK)):
        qc, trimmed = ReadQc(), ReadQc()
        assert scan_single_end_files(*args, **kwargs, qc=qc) == scan_single_end_files(*args, **kwargs)
        _same_result(qc.result(), f["before"][:1], f["before"][:1], None)   # no pairs: no insert sizes
        cfg = _route_config()
        assert scan_single_end_files(*args, **kwargs, adapter_trim=cfg, qc=trimmed) == \
            scan_single_end_files(*args, **kwargs, adapter_trim=cfg)
        _same_result(trimmed.result(), f["before"][:1], [f["after_single"]], None)


@pytest.mark.gpu
def test_streamed_multi_csv_measures_once(files):
    from genefuserust_amd.multi_csv_scan import scan_multi_csv_report
    from genefuserust_amd.read_qc import ReadQc
    f = files
    for chunk_bytes in (CHUNK, None):
        qc = ReadQc()
        got = scan_multi_csv_report(f["fa"], f["two"], f["r1"], f["r2"], chunk_bytes=chunk_bytes, qc=qc)
        want = scan_multi_csv_report(f["fa"], f["two"], f["r1"], f["r2"], chunk_bytes=chunk_bytes)
        assert len(got) == 2 and [(c, r, k) for c, r, k in got] == [(c, r, k) for c, r, k in want]
        _same_result(qc.result(), f["before"], f["before"], f["inserts"])   # two CSVs, one measurement


@pytest.mark.gpu
def test_a_second_device_and_a_lean_cut_are_refused(ix):
    import torch
    qc = read_qc.ReadQc()
    b = _batch(list(_mixed()[:5]))
    qc.measure(ix, "before", b)
    assert np.array_equal(qc.result().before[0], stats_table(list(_mixed()[:5])))
    with pytest.raises(ValueError, match="full FASTQ cut"):
        qc.measure(ix, "before", b._replace(qual_off=b.offsets))

    class _Elsewhere:
        def info(self):
            return {"device": torch.cuda.current_device() + 1}
    with pytest.raises(ValueError, match="one of its own"):
        qc.measure(_Elsewhere(), "before", b)
