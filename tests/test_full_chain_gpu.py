"""The pair routes with all seven steps on at once — ``umi``, ``overlap_correct``, ``adapter_trim``, ``read_filter``,
``dedup``, ``qc`` and ``write_reads`` — against the chain of the Python models the suite already has, run in the route's
order: ``umi_model.cut``, ``overlap_correct_model.correct_batch``, ``adapter_trim_model.trim_batch``,
``read_filter_model.filter_batch``, ``umi_model.dedup_keys`` with ``dedup_model.Table``, and
``read_write_model.format_reads``; QC "before" over the records as read and "after" over what the removal leaves
(``read_qc_model``).  The overlap correction is the step the other route modules do not combine with the UMI cut (which
moves every record's start), with ``qc`` or with ``write_reads``.

The fixture is that of tests/test_read_write_gpu.py — molecules under inline UMIs, second molecules, PCR copies in the
other letter case, two pairs too short for the UMI — over the records of
``tests.test_overlap_correct_gpu._corrected_files``, whose overlaps carry low-quality miscalls; every PCR copy gets one
more such miscall, so that it is a duplicate only once it has been corrected; and a few pairs over a tandem repeat make
the order of correction and trimming visible (``_order_pairs``).  A test without a GPU holds the fixture to what it is
for, on the models alone: the same chain without the correction, or with the correction behind the trimming, writes
another text, finds other duplicates and measures another QC table, so a route that skips or misplaces the step cannot
pass."""
import gzip
import os

import numpy as np
import pytest

from genefuserust_amd import dedup as dd
from genefuserust_amd import read_write as rw
from genefuserust_amd import umi as um
from genefuserust_amd.adapter_trim import ADAPTER_COUNTER_KEYS
from genefuserust_amd.overlap_correct import CORRECT_COUNTER_KEYS
from genefuserust_amd.read_filter import COUNTER_KEYS as FILTER_COUNTER_KEYS
from genefuserust_amd.read_write import ReadWriter
from genefuserust_amd.umi import Umi
from tests import dedup_model, read_qc_model, umi_model
from tests import read_write_model as model
from tests.adapter_trim_cases import rc
from tests.adapter_trim_model import accepted_inserts, complementary, trim_batch
from tests.overlap_correct_model import correct_batch, correct_pair, insert_of, phred
from tests.read_filter_model import filter_batch
from tests.test_adapter_trim_gpu import ROUTE_SETTINGS as TRIM_SETTINGS
from tests.test_overlap_correct_gpu import ROUTE_SETTINGS as CORRECT_SETTINGS
from tests.test_overlap_correct_gpu import _config, _corrected_files, _miscall
from tests.test_read_qc_gpu import _same_result
from tests.test_read_write_gpu import CHUNK, LENGTH, SKIP, ROOT, _read, _records, _texts, _write
from tests.umi_cases import random_bases

STEP_KEYS = (um.UMI_COUNTER_KEYS + CORRECT_COUNTER_KEYS + ADAPTER_COUNTER_KEYS + FILTER_COUNTER_KEYS
             + dd.DEDUP_COUNTER_KEYS + rw.WRITE_COUNTER_KEYS)
GOOD = CORRECT_SETTINGS.good_phred


def _order_pairs(count: int = 3):
    """Pairs on which it shows whether the correction ran ahead of the trimming: mates of 150 bases over a fragment
    of 160 that repeats a unit of 40 bases, so that every insert 40, 80 .. 240 is a candidate.  Five good calls that
    disagree in R1[120:150) and one low-quality miscall in R1[90:120) give the inserts 160, 200 and 240 six differences,
    one too many; R1[120:150) faces nothing at the insert 120, which has the miscall alone and is the largest accepted.
    The correction at 120 rewrites the miscall, the larger inserts come under the limit, and the trimming behind it
    keeps all 150 bases; a trimming ahead of the correction cuts both mates to 120.  Asserted here, on the models."""
    rng = np.random.default_rng(123)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for k in range(count):
        frag = bytes(rng.choice(letters, 40)) * 4
        l = [b"@order%d/1" % k, frag[:150], b"+", b"F" * 150]
        r = [b"@order%d/2" % k, rc(frag)[:150], b"+", b"F" * 150]
        for at in rng.choice(np.arange(120, 150), 5, replace=False):
            _miscall(l, int(at), ord("F"))
        _miscall(l, int(rng.integers(90, 120)), ord("#"))
        before = accepted_inserts(l[1], r[1], TRIM_SETTINGS)
        c = correct_pair(l[1], l[3], r[1], r[3], CORRECT_SETTINGS)
        after = accepted_inserts(c.a, c.b, TRIM_SETTINGS)
        assert max(before) == c.insert == 120 and max(after) == 240 and c.fixed == (1, 0) and c.left == 0
        out.append((l, r))
    return out


def _copy_with_a_miscall(rng, l, r, to_r1: bool):
    """The records of a PCR copy: one more miscall of low quality inside the overlap, in R1 or in R2, at a place where
    the mates agree and both calls are good — so that the corrected copy is the corrected original.  None when the pair
    has no overlap or no such place."""
    s = CORRECT_SETTINGS
    insert = insert_of(l[1], r[1], s)
    if insert < 0:
        return None
    want = correct_pair(l[1], l[3], r[1], r[3], s)
    lo, hi = max(0, insert - len(r[1])), min(insert, len(l[1]))
    for i in (int(x) for x in rng.permutation(np.arange(lo, hi))):
        j = insert - 1 - i
        if not complementary(l[1][i], r[1][j]) or phred(l[3][i]) < GOOD or phred(r[3][j]) < GOOD:
            continue
        cl, cr = list(l), list(r)
        _miscall(cl, i, ord("#")) if to_r1 else _miscall(cr, j, ord("#"))
        got = correct_pair(cl[1], cl[3], cr[1], cr[3], s)
        if (got.a, got.b) == (want.a, want.b) and (cl[1], cr[1]) != (l[1], r[1]):
            return cl, cr
    return None


def model_chains(texts, originals, fs) -> dict:
    """What the seven steps leave, from the models, with the correction where the routes have it ("route": behind the
    UMI cut, ahead of the trimming), behind the trimming ("late") and nowhere ("never").  What the three share — the
    cut, the trimming of uncorrected records, QC "before" — is computed once."""
    cut = umi_model.cut(model.PER_READ, LENGTH, SKIP, list(zip(*originals)))
    cut_lists = [[r[s] for r in cut.records] for s in (0, 1)]
    before = [read_qc_model.stats_table(side) for side in originals]
    inserts = read_qc_model.insert_hist([(a[0], b[0]) for a, b in zip(*originals)])
    trimmed_uncorrected = trim_batch(cut_lists[0], cut_lists[1], TRIM_SETTINGS)
    out = {}
    for how in ("route", "late", "never"):
        corrected, trimmed = None, trimmed_uncorrected
        if how == "route":
            corrected = correct_batch(cut_lists[0], cut_lists[1], CORRECT_SETTINGS)
            trimmed = trim_batch(corrected.reads[0], corrected.reads[1], TRIM_SETTINGS)
        lists = trimmed.reads
        if how == "late":
            corrected = correct_batch(lists[0], lists[1], CORRECT_SETTINGS)
            lists = corrected.reads
        kept = filter_batch(lists[0], lists[1], fs)
        cleaned = list(zip(*kept.reads))
        keys = umi_model.dedup_keys(cleaned, cut.codes)
        table = dedup_model.Table()
        dd_totals = table.insert(keys, 0)
        dup = table.duplicates(keys, 0)
        removed = sum(len(a[0]) + len(b[0]) for (a, b), d in zip(cleaned, dup) if d)
        finals = [[(b"", b"") if d else r for r, d in zip(side, dup)] for side in kept.reads]
        counters = dict(zip(um.UMI_COUNTER_KEYS, cut.totals[1:6]))
        if corrected is not None:
            counters.update(corrected.counters())
        counters.update(trimmed.counters())
        counters.update(kept.counters())
        counters.update(zip(dd.DEDUP_COUNTER_KEYS, (dd_totals[1], dd_totals[2], sum(dup), removed)))
        out[how] = dict(corrected=corrected, dup=dup, finals=finals, counters=counters, before=before, inserts=inserts,
                        plain=model.format_reads(texts, finals),
                        tagged=model.format_reads(texts, finals, model.PER_READ, LENGTH, originals),
                        after=[read_qc_model.stats_table(side) for side in finals])
    return out


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """Host only: the files, and what the chain of models leaves of them — in the route's order, with the correction
    behind the trimming, and without it."""
    tmp = tmp_path_factory.mktemp("full_chain")
    f = _corrected_files(tmp)
    golden = os.path.join(ROOT, "tests", "golden")
    extra = _order_pairs()
    base = [_records(os.path.join(golden, "R1.fq")) + _records(f["r1"]) + [l for l, _ in extra],
            _records(os.path.join(golden, "R2.fq")) + _records(f["r2"]) + [r for _, r in extra]]
    n = len(base[0])
    assert n == len(base[1]) == 153 + len(extra)
    rng = np.random.default_rng(78)
    umis = [(random_bases(rng, LENGTH), random_bases(rng, LENGTH)) for _ in range(n)]
    order = [(k, "A") for k in range(n)] + [(k, "molB") for k in range(0, n, 4)] + [(k, "copy") for k in range(0, n, 3)]
    order += [(1, "short"), (2, "short")]
    sides, miscalled = [[], []], 0
    for at, (k, kind) in enumerate(order):
        u = umis[k]
        if kind == "molB":
            u = (u[0][::-1] + b"", u[1][:-1] + (b"A" if u[1][-1:] not in b"Aa" else b"C"))
        lower = kind == "copy"
        records = [base[0][k], base[1][k]]
        if kind == "copy":
            changed = _copy_with_a_miscall(rng, *records, to_r1=at % 2 == 0)
            if changed is not None:
                records, miscalled = changed, miscalled + 1
        for side in (0, 1):
            name, seq, plus, qual = records[side]
            tag = b"" if kind == "A" else b" " + kind.encode()
            prefix = (u[side].swapcase() if lower else u[side]) + b"TG"
            if kind == "short" and side == k - 1:
                sides[side].append([name + tag, prefix[:7], plus, b"I" * 7])
            else:
                sides[side].append([name + tag, prefix + (seq.swapcase() if lower else seq), plus, b"I" * 10 + qual])
    for key, side, nl in (("w1", sides[0], True), ("w2", sides[1], False)):
        f[key] = str(tmp / (key + ".fq"))
        _write(f[key], side, nl)
    f["order"], f["miscalled_copies"] = order, miscalled
    f["texts"] = [_read(f[key]) for key in ("w1", "w2")]
    two = tmp / "two.txt"
    two.write_text("%s\n%s\n" % (f["csvs"][3], f["csvs"][0]))
    f["two"] = str(two)
    originals = [[(r[1], r[3]) for r in side] for side in sides]
    f.update(model_chains(f["texts"], originals, f["fs"]))
    # the model's final records as files of their own: what a scan with no step is given for comparison
    for key, text in zip(("fin1", "fin2"), f["route"]["plain"].texts):
        f[key] = str(tmp / (key + ".fq"))
        with open(f[key], "wb") as fh:
            fh.write(text)
    return f


def _steps(f):
    """All six steps in front of the writer, each a fresh object."""
    from genefuserust_amd.read_filter import ReadFilter
    from genefuserust_amd.read_qc import ReadQc
    from tests.test_adapter_trim_gpu import _route_config
    return dict(umi=Umi("per_read", LENGTH, SKIP), overlap_correct=_config(CORRECT_SETTINGS), adapter_trim=_route_config(),
                read_filter=ReadFilter(*f["fs"]), dedup=dd.Dedup(slots=1024), qc=ReadQc())


# ---- without a GPU: the fixture is worth its name ----------------------------------------------------------------------

def test_the_correction_changes_text_duplicates_and_qc(chain):
    f = chain
    want, late, never = f["route"], f["late"], f["never"]
    assert all(t > 0 for t in want["corrected"].totals), want["corrected"].totals     # every total of the correction
    kinds = [kind for _, kind in f["order"]]
    assert f["miscalled_copies"] > 20 and kinds.count("copy") > f["miscalled_copies"]
    for other in (never, late):
        for side in (0, 1):
            assert other["plain"].texts[side] != want["plain"].texts[side]
            assert other["tagged"].texts[side] != want["tagged"].texts[side]
        assert other["counters"] != want["counters"]
    # without the correction a miscalled copy is no duplicate: fewer duplicates, and other ones
    assert never["dup"] != want["dup"] and sum(never["dup"]) <= sum(want["dup"]) - f["miscalled_copies"]
    assert [bool(d) for d in want["dup"]] == [kind == "copy" for kind in kinds]     # behind it: the copies, and only they
    # ... and the "after" tables differ where qualities are counted (QUAL_SUM, Q20, Q30 of the cycle rows)
    for side in (0, 1):
        a, b = (x["after"][side][513:].reshape(513, 8)[:, read_qc_model.QUAL_SUM:] for x in (want, never))
        assert not np.array_equal(a, b)
        assert np.array_equal(want["before"][side], never["before"][side])
    assert any(not np.array_equal(late["after"][s], want["after"][s]) for s in (0, 1))
    # every step does something, and the writer has records to drop
    c = want["counters"]
    assert list(c) == list(STEP_KEYS[:-3])
    for k in ("umi_reads_tagged", "umi_too_short", "corrected_bases", "adapter_reads_cut", "reads_too_short",
              "dedup_duplicates", "dedup_bases_removed"):
        assert c[k] > 0, k
    assert sum(c[k] for k in ("reads_too_short", "reads_too_many_n", "reads_low_quality", "reads_mate_failed")) > 0
    assert want["plain"].totals[0] > 100 and want["plain"].totals[4] > 40
    assert want["inserts"][30:1025].sum() >= 20
    # what is written is consistent: scanned again under its tags, nothing is left to correct and no duplicate is left
    written = [[r for r, w in zip(side, want["tagged"].written) if w] for side in want["finals"]]
    again = correct_batch(written[0], written[1], CORRECT_SETTINGS)
    assert again.totals[0] == want["plain"].totals[0] and again.totals[4] == 0 and again.totals[1] > 0
    codes, totals = umi_model.names(want["tagged"].texts[0], len(written[0]))
    assert totals[2] == 0
    keys = umi_model.dedup_keys(list(zip(*again.reads)), codes)
    assert len(set(keys)) == len(keys)


# ---- the routes ---------------------------------------------------------------------------------------------------------

def _same_counters(got: dict, f, formatted):
    """Every step's keys are its model's, and they stand in the order the routes owe."""
    want = dict(f["route"]["counters"], **model.counters(formatted.totals))
    assert {k: got[k] for k in STEP_KEYS} == want
    keys = list(got)
    at = keys.index(STEP_KEYS[0])
    assert tuple(keys[at:at + len(STEP_KEYS)]) == STEP_KEYS


def _names_and_reads(matches):
    return [(m.m_name, m.m_read) for m in matches]


@pytest.fixture(scope="module")
def plain_scans(chain, gpu_device):
    """The scans with no step over the files of the model's final records, each made once."""
    from genefuserust_amd.scan import scan_pair_end_files, scan_pair_end_report
    args = (chain["fa"], chain["csvs"][3], chain["fin1"], chain["fin2"])
    return {"files": scan_pair_end_files(*args), "report": scan_pair_end_report(*args)}


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["files", "report"])
def test_pair_route_one_chunk_and_many(gpu_device, chain, plain_scans, tmp_path, route):
    from genefuserust_amd import scan
    f, want = chain, chain["route"]
    call = {"files": scan.scan_pair_end_files, "report": scan.scan_pair_end_report}[route]
    args = (f["fa"], f["csvs"][3], f["w1"], f["w2"])
    plain = plain_scans[route]
    assert len(plain[0]) > 0
    outs, results = {}, {}
    for name, chunk_bytes in (("one", 1 << 22), ("many", CHUNK)):
        steps = _steps(f)
        w = ReadWriter(str(tmp_path / (name + "_1.fq")), str(tmp_path / (name + "_2.fq")))
        got = call(*args, chunk_bytes=chunk_bytes, **steps, write_reads=w)
        assert (got[1]["chunks"] == 1) if name == "one" else (got[1]["chunks"] >= 3)
        outs[name] = (_read(w.out1), _read(w.out2))
        assert outs[name] == tuple(want["plain"].texts), name                # byte for byte
        _same_counters(got[1], f, want["plain"])
        _same_result(steps["qc"].result(), want["before"], want["after"], want["inserts"])
        assert steps["dedup"].result().duplicates == sum(want["dup"])
        r = w.result()
        assert (r.records, r.bases, r.bytes, r.not_written) == (
            want["plain"].totals[0], want["plain"].totals[1], tuple(want["plain"].totals[2:4]), want["plain"].totals[4])
        # what is found is what a scan with no step finds in the model's final records
        if route == "report":
            assert _texts(got[0]) == _texts(plain[0])
        else:
            assert _names_and_reads(got[0]) == _names_and_reads(plain[0])
        assert got[1]["pairs"] == len(f["order"]) and plain[1]["pairs"] == want["plain"].totals[0]
        results[name] = got
    assert outs["one"] == outs["many"]
    rest = [{k: v for k, v in results[name][1].items() if k != "chunks"} for name in ("one", "many")]
    assert rest[0] == rest[1] and list(rest[0]) == list(rest[1])
    assert results["one"][0] == results["many"][0]


@pytest.mark.gpu
def test_pair_route_tagged_names_deflated_on_the_device(gpu_device, chain, plain_scans, tmp_path):
    from genefuserust_amd.scan import scan_pair_end_report
    from genefuserust_amd import deflate as df
    from tests.test_deflate_gpu import _markers
    f, want = chain, chain["route"]
    args = (f["fa"], f["csvs"][3], f["w1"], f["w2"])
    got, outs, qcs = {}, {}, {}
    for how in ("host", "device"):
        steps = _steps(f)
        w = ReadWriter(str(tmp_path / (how + "_1.fq.gz")), str(tmp_path / (how + "_2.fq.gz")), umi_in_name=True, deflate=how)
        got[how] = scan_pair_end_report(*args, chunk_bytes=CHUNK, **steps, write_reads=w)
        outs[how], qcs[how] = w, steps["qc"]
    assert got["device"][1]["chunks"] >= 3
    assert got["device"][1] == got["host"][1] and list(got["device"][1]) == list(got["host"][1])     # every counter
    _same_counters(got["device"][1], f, want["tagged"])
    assert _texts(got["device"][0]) == _texts(got["host"][0]) == _texts(plain_scans["report"][0])
    _same_result(qcs["device"].result(), want["before"], want["after"], want["inserts"])
    for side, (h, d) in enumerate(zip(outs["host"].outputs, outs["device"].outputs)):
        assert gzip.decompress(_read(d)) == want["tagged"].texts[side]
        assert gzip.decompress(_read(h)) == want["tagged"].texts[side]
        members, empty, ends = _markers(d)
        assert members >= 4 and empty == 1 and ends          # it walks as BGZF; exactly one marker, at the end
        assert outs["device"].compressed_bytes[side] == os.path.getsize(d) - len(df.EOF_MARKER)
    assert outs["device"].result() == outs["host"].result()
    assert outs["device"].result().bytes == tuple(want["tagged"].totals[2:4])


@pytest.mark.gpu
def test_two_csvs_write_once(gpu_device, chain, tmp_path):
    from genefuserust_amd.multi_csv_scan import scan_multi_csv_report
    from genefuserust_amd.scan import scan_pair_end_report
    f, want = chain, chain["route"]
    steps = _steps(f)
    w = ReadWriter(str(tmp_path / "m1.fq"), str(tmp_path / "m2.fq"))
    got = scan_multi_csv_report(f["fa"], f["two"], f["w1"], f["w2"], chunk_bytes=CHUNK, **steps, write_reads=w)
    assert len(got) == 2 and [g[0] for g in got] == [f["csvs"][3], f["csvs"][0]]
    assert (_read(w.out1), _read(w.out2)) == tuple(want["plain"].texts)          # written once, and the model's
    assert w.result().records == want["plain"].totals[0]
    for _, results, counters in got:
        assert counters["chunks"] >= 3
        _same_counters(counters, f, want["plain"])                               # the same step totals for every CSV
    _same_result(steps["qc"].result(), want["before"], want["after"], want["inserts"])   # two CSVs, one measurement
    assert steps["dedup"].offered == len(f["order"])
    for (csv, results, _) in got:
        plain = scan_pair_end_report(f["fa"], csv, f["fin1"], f["fin2"])
        assert _texts(results) == _texts(plain[0])
    assert sum(1 for g in got if len(g[1]) > 0) >= 1


@pytest.mark.gpu
def test_round_trip_nothing_left_to_correct_or_remove(gpu_device, chain, tmp_path):
    """The tagged files scanned again with the UMIs read from the names, the removal and the correction: what was
    written is already consistent."""
    from genefuserust_amd.scan import scan_pair_end_files
    f, want = chain, chain["route"]
    args = (f["fa"], f["csvs"][3])
    w = ReadWriter(str(tmp_path / "t1.fq"), str(tmp_path / "t2.fq"), umi_in_name=True)
    first = scan_pair_end_files(*args, f["w1"], f["w2"], chunk_bytes=CHUNK, **_steps(f), write_reads=w)
    assert (_read(w.out1), _read(w.out2)) == tuple(want["tagged"].texts)
    second = scan_pair_end_files(*args, w.out1, w.out2, umi=Umi("name"), dedup=dd.Dedup(slots=1024),
                                 overlap_correct=_config(CORRECT_SETTINGS))
    assert second[1]["pairs"] == first[1]["written_records"] == second[1]["umi_reads_tagged"] == want["tagged"].totals[0]
    assert second[1]["umi_missing"] == 0 and second[1]["dedup_duplicates"] == 0
    assert second[1]["dedup_unique"] == second[1]["pairs"]
    assert second[1]["corrected_bases"] == 0 and second[1]["corrected_reads"] == 0
    assert second[1]["correction_overlapping_pairs"] > 0
    assert [m.m_read for m in second[0]] == [m.m_read for m in first[0]] and len(first[0]) > 0
