"""libgfwrite.so on the device (include/gf_read_write.h): ``gf_rw_format_device`` against the model
(tests/read_write_model.py), byte for byte — text, offsets and totals, with every buffer inside junk that must stay —,
every streamed route of a scan with ``write_reads`` against the models of the five steps in front of it, and the
written files scanned again."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from genefuserust_amd import dedup as dd
from genefuserust_amd import read_write as rw
from genefuserust_amd import umi as um
from genefuserust_amd.read_write import ReadWriter
from genefuserust_amd.umi import Umi
from tests import dedup_model, umi_model
from tests import read_write_model as model
from tests.read_write_cases import KEPT, KEPT_SMALL, UMI_LENGTHS, build
from tests.umi_cases import random_bases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 255, 256, 257, 600]
GUARD, JUNK = 64, 0xA5


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


def _placed(data: bytes, lead: int, rng):
    """``data`` on the device with ``lead`` + 64 bytes of junk in front and 64 behind: (the whole tensor, the address of
    the first byte of ``data``, which lies ``lead`` bytes behind a 16-byte boundary)."""
    front = GUARD + lead      # (the allocator's blocks are aligned to far more than 16 bytes)
    whole = _up(bytes(rng.integers(0, 256, front, dtype=np.uint8)) + data + bytes(rng.integers(0, 256, GUARD, dtype=np.uint8)))
    assert whole.data_ptr() % 16 == 0
    return whole, whole.data_ptr() + front


def _format(ix, texts, finals, pre, source=model.NAME, length=0, gather=model.WIDE, leads=None, seed=0):
    """One raw ``gf_rw_format_device`` call with every buffer inside junk: (texts, offsets, totals) as the call left
    them, after the checks that the inputs and the junk around everything stayed.  ``leads``: per side the alignments
    (0 .. 15) of the first byte of the text, the records, the pre-cut records and the output."""
    import torch
    rng = np.random.default_rng(seed)
    sides, n = len(texts), len(finals[0])
    leads = leads or [(0, 0, 0, 0)] * sides
    tagged = source != model.NAME
    structs, held, outs = [], [], []
    for s in range(sides):
        a_text, a_rec, a_pre, a_out = leads[s]
        text = texts[s]
        nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10).astype(np.int64)
        d_nl = torch.from_numpy(nl).cuda()
        t_whole, t_ptr = _placed(text, a_text, rng)
        b_whole, b_ptr = _placed(b"".join(b for b, _ in finals[s]), a_rec, rng)
        q_whole, q_ptr = _placed(b"".join(q for _, q in finals[s]), (a_rec + 5) % 16, rng)   # (an alignment of its own)
        off = np.concatenate([[0], np.cumsum([len(b) for b, _ in finals[s]], dtype=np.int64)]).astype(np.int64)
        d_off = torch.from_numpy(off).cuda()
        ins = [t_whole, b_whole, q_whole, d_off, d_nl]
        p_ptr = po_ptr = None
        if tagged:
            p_whole, p_ptr = _placed(b"".join(b for b, _ in pre[s]), a_pre, rng)
            p_off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(b) for b, _ in pre[s]], dtype=np.int64)])
                                     .astype(np.int64)).cuda()
            po_ptr = p_off.data_ptr()
            ins += [p_whole, p_off]
        cap = model.capacity(len(text), n)
        out = torch.full((GUARD + a_out + cap + GUARD,), JUNK, dtype=torch.uint8, device="cuda")
        out_off = torch.full((n + 1 + 8,), -77, dtype=torch.int64, device="cuda")
        structs.append(rw.GfRwSide(t_ptr if text else None, len(text), d_nl.data_ptr() if len(nl) else None, len(nl),
                                   b_ptr, q_ptr, d_off.data_ptr(), p_ptr, po_ptr, out.data_ptr() + GUARD + a_out, cap,
                                   out_off.data_ptr()))
        held.append([(t, t.clone()) for t in ins])
        outs.append((out, out_off, GUARD + a_out, cap))
    L = rw.lib()
    ws_bytes = int(L.gf_rw_workspace_bytes(n))
    ws = torch.full((ws_bytes + GUARD,), 0x3C, dtype=torch.uint8, device="cuda")
    before = [1000, 0, 5, 0, 7]
    totals = torch.tensor(before, dtype=torch.int64, device="cuda")
    settings = rw.GfRwSettings(source, length, gather)
    rw.check(L.gf_rw_format_device(ix._handle(), C.addressof(settings), C.addressof(structs[0]),
                                   C.addressof(structs[1]) if sides == 2 else None, n, ws.data_ptr(), ws_bytes,
                                   totals.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for side in held:
        for t, t0 in side:
            assert torch.equal(t, t0)
    assert (ws.cpu().numpy()[ws_bytes:] == 0x3C).all()
    got_texts, got_offsets = [], []
    for out, out_off, first, cap in outs:
        off = out_off.cpu().numpy()
        assert (off[n + 1:] == -77).all()
        total = int(off[n])
        assert 0 <= total <= cap
        o = out.cpu().numpy()
        assert (o[:first] == JUNK).all() and (o[first + total:] == JUNK).all()      # nothing outside the text
        got_texts.append(o[first:first + total].tobytes())
        got_offsets.append([int(x) for x in off[:n + 1]])
    return got_texts, got_offsets, [a - b for a, b in zip(totals.cpu().tolist(), before)]


def _against_the_model(ix, texts, finals, pre, source=model.NAME, length=0, gather=model.WIDE, leads=None, seed=0):
    want = model.format_reads(texts, finals, source, length, pre)
    got = _format(ix, texts, finals, pre, source, length, gather, leads, seed)
    assert got[2] == want.totals
    assert got[1] == want.offsets
    for g, w in zip(got[0], want.texts):
        assert g == w
    return want


# ---- the call against the model -----------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("gather", [model.WIDE, model.BYTES])
def test_batch_sizes(ix, gather):
    """Every batch size around the tile, every kept length of the cases (0, 1, 15, 16, 17, 31, 32, 33, 150, 151 and
    5000, above GF_MAX_READ_LEN) under names of 2, 15, 16, 17, 255, 256 and 257 bytes with and without a space, a tab
    or a '\\r', pairs whose mates are out of step, then reads; texts with and without their final newline."""
    written = dropped = 0
    for n in SIZES:
        rng = np.random.default_rng(100 + n)
        kept = KEPT if n in (257, 600) else KEPT_SMALL
        texts, finals, pre = build(rng, n, 2, final_newline=n % 2 == 0, kept=kept)
        want = _against_the_model(ix, texts, finals, pre, gather=gather, leads=[(n % 16, 3, 0, (n + 5) % 16), (9, n % 13, 0, 1)],
                                  seed=n)
        assert want.totals[0] + want.totals[4] == n and want.totals[2] == len(want.texts[0])
        written, dropped = written + want.totals[0], dropped + want.totals[4]
        if n >= 255:
            lens = [(len(l[0]), len(r[0])) for l, r in zip(*finals)]
            assert any(x == 0 and y > 0 for x, y in lens) and any(x > 0 and y == 0 for x, y in lens)
        texts, finals, pre = build(rng, n, 1, final_newline=n % 2 == 1, kept=kept)
        single = _against_the_model(ix, texts, finals, pre, gather=gather, leads=[((5 * n) % 16, 7, 0, (3 * n) % 16)], seed=n)
        written, dropped = written + single.totals[0], dropped + single.totals[4]
    assert written > 500 and dropped > 100


@pytest.mark.gpu
@pytest.mark.parametrize("gather", [model.WIDE, model.BYTES])
def test_every_alignment(ix, gather):
    """The texts, the batches and the outputs laid at every alignment 0 .. 15 of the first byte, both sides at
    different ones; the first record at byte 0 of its text."""
    rng = np.random.default_rng(7)
    written = dropped = 0
    for lead in range(16):
        texts, finals, pre = build(rng, 23, 2, final_newline=lead % 2 == 0, kept=KEPT_SMALL)
        leads = [(lead, (3 * lead + 5) % 16, 0, (7 * lead + 1) % 16), ((lead + 8) % 16, (5 * lead) % 16, 0, (15 - lead))]
        want = _against_the_model(ix, texts, finals, pre, gather=gather, leads=leads, seed=lead)
        # ... and the output at this alignment too, the inputs at others
        _against_the_model(ix, texts, finals, pre, gather=gather, leads=[(3, 11, 0, lead), (6, 2, 0, lead)], seed=lead)
        written, dropped = written + want.totals[0], dropped + want.totals[4]
        assert want.offsets[0][0] == 0 and texts[0][:1] == b"@"
    assert written > 50 and dropped > 50


@pytest.mark.gpu
@pytest.mark.parametrize("source", [model.READ1, model.READ2, model.PER_READ])
def test_tags(ix, source):
    """The tag of every inline source at the UMI lengths 1, 8 and 32, pairs and (but for read2) reads, wide and plain,
    the pre-cut batches at alignments of their own; both mates carry the same tag, in the case the bases had."""
    rng = np.random.default_rng(20 + source)
    written = dropped = 0
    tags = b""
    for k, length in enumerate(UMI_LENGTHS):
        for sides in (2, 1):
            if sides == 1 and source == model.READ2:
                continue
            texts, finals, pre = build(rng, 40, sides, source, length, skip=k, final_newline=k % 2 == 0, kept=KEPT_SMALL)
            leads = [((k + 4 * s) % 16, (3 * k + s) % 16, (5 * k + 9 * s + 1) % 16, (11 * k + 3 * s) % 16)
                     for s in range(sides)]
            for gather in (model.WIDE, model.BYTES):
                want = _against_the_model(ix, texts, finals, pre, source, length, gather, leads, seed=k)
            written, dropped = written + want.totals[0], dropped + want.totals[4]
            i = want.written.index(True)
            t = model.tag(source, length, [p[i][0] for p in pre])
            assert len(t) == (2 + 2 * length if source == model.PER_READ and sides == 2 else 1 + length)
            for s in range(sides):
                name = want.texts[s][want.offsets[s][i]:want.offsets[s][i + 1]].split(b"\n")[0]
                assert t in name and len(name) == len(model.name_line(texts[s], i)) + len(t)
            tags += t
    assert written > 30 and dropped > 10
    assert any(c in tags for c in b"acgt") and any(c in tags for c in b"ACGT")      # the case is kept


@pytest.mark.gpu
def test_all_dropped_no_records_and_names_past_the_text(ix):
    q = b"F" * 8
    text = b"@a\nACGTACGT\n+\nFFFFFFFF\n@b\nAC\n+\nFF\n"
    none = [(b"", b""), (b"", b"")]
    got = _format(ix, [text], [none], [none])
    assert got == ([b""], [[0, 0, 0]], [0, 0, 0, 0, 2])            # an all-dropped batch: 0 bytes out
    got = _format(ix, [text, text], [[(b"ACGTACGT", q), (b"", b"")], none[:1] + [(b"AC", q[:2])]], [none, none])
    assert got == ([b"", b""], [[0, 0, 0]] * 2, [0, 0, 0, 0, 2])   # only R2 empty, only R1 empty: neither is written
    assert _format(ix, [b""], [[]], [[]]) == ([b""], [[0]], [0, 0, 0, 0, 0])
    # a record whose name line the text does not have is written under an empty name; a text that ends in a name line
    for t in (text, text + b"@last"):
        three = [(b"ACGTACGT", q), (b"AC", q[:2]), (b"GG", q[:2])]
        want = _against_the_model(ix, [t], [three], [three], leads=[(5, 6, 0, 7)])
        assert want.texts[0].endswith((b"\nGG\n+\nFF\n")) and want.totals[:2] == [3, 12]
    assert want.texts[0].endswith(b"@last\nGG\n+\nFF\n")
    # the known answer of the header
    got = _format(ix, [b"@r1 x\nACGT\n+\nFFFF\n"], [[(b"GT", b"FF")]], [[(b"ACGT", b"FFFF")]], model.READ1, 2)
    assert got[0] == [b"@r1:AC x\nGT\n+\nFF\n"]


@pytest.mark.gpu
def test_the_binding_formats_what_the_cut_and_the_umi_step_leave(ix):
    """``format_reads_device`` over ``fastq_cut_device`` and ``cut_umis_device``: the text of the cut records under
    tagged names, and without a tag the text as it came, but for the records without bases."""
    from genefuserust_amd.fastq import fastq_cut_device
    rng = np.random.default_rng(3)
    texts, _, originals = build(rng, 300, 2, model.PER_READ, 8, 2, kept=KEPT_SMALL)
    d_texts = [_up(t) for t in texts]
    cuts = [fastq_cut_device(ix, t) for t in d_texts]
    assert all(int(c.n_records) == 300 for c in cuts)
    *kept, codes, _ = um.cut_umis_device(ix, Umi("per_read", 8, 2), *cuts)
    out_texts, out_offs, totals = rw.format_reads_device(ix, d_texts, cuts, kept, 300, pre=cuts, umi=Umi("per_read", 8, 2))
    cut = umi_model.cut(model.PER_READ, 8, 2, list(zip(*originals)))
    finals = [[r[s] for r in cut.records] for s in (0, 1)]
    want = model.format_reads(texts, finals, model.PER_READ, 8, originals)
    assert totals.cpu().tolist() == want.totals and want.totals[0] > 0 and want.totals[4] > 0
    for s in (0, 1):
        off = out_offs[s].cpu().tolist()
        assert off == want.offsets[s] and out_texts[s][:off[-1]].cpu().numpy().tobytes() == want.texts[s]
        assert out_texts[s].numel() == rw.capacity(len(texts[s]), 300)
    # no step at all: the records with bases in both mates, as they came
    out_texts, out_offs, totals = rw.format_reads_device(ix, d_texts, cuts, cuts, 300)
    plain = model.format_reads(texts, originals)
    for s in (0, 1):
        assert out_texts[s][:int(out_offs[s][-1])].cpu().numpy().tobytes() == plain.texts[s]
    # the first 100 records only: what a chunk that carries the rest over writes
    out_texts, out_offs, totals = rw.format_reads_device(ix, d_texts, cuts, cuts, 100)
    part = model.format_reads(texts, [o[:100] for o in originals])
    assert totals.cpu().tolist() == part.totals
    assert out_texts[1][:int(out_offs[1][-1])].cpu().numpy().tobytes() == part.texts[1]


@pytest.mark.gpu
def test_host_memory_behind_any_pointer_is_refused(ix):
    """A host array where the kernels would read or write is ``GF_ERR_NO_DEVICE``, and nothing is launched."""
    import torch
    from genefuserust_amd import _lib
    rng = np.random.default_rng(2)
    texts, finals, pre = build(rng, 5, 1, model.READ1, 8, kept=[20, 30])
    n = 5
    d_text = _up(texts[0])
    nl = torch.from_numpy(np.flatnonzero(np.frombuffer(texts[0], dtype=np.uint8) == 10).astype(np.int64)).cuda()
    bases, quals = _up(b"".join(b for b, _ in finals[0])), _up(b"".join(q for _, q in finals[0]))
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(b) for b, _ in finals[0]])]).astype(np.int64)).cuda()
    p_bases = _up(b"".join(b for b, _ in pre[0]))
    p_off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(b) for b, _ in pre[0]])]).astype(np.int64)).cuda()
    cap = rw.capacity(len(texts[0]), n)
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    out_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    L, h = rw.lib(), ix._handle()
    ws_bytes = int(L.gf_rw_workspace_bytes(n))
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
    totals = torch.zeros(rw.TOTALS, dtype=torch.int64, device="cuda")
    host = torch.zeros(max(cap, ws_bytes) // 8 + 8, dtype=torch.int64)
    good = dict(d_text=d_text, d_nl_pos=nl, d_bases=bases, d_quals=quals, d_off=off, d_pre_bases=p_bases, d_pre_off=p_off,
                d_out_text=out, d_out_off=out_off, ws=ws, totals=totals)
    settings = rw.GfRwSettings(model.READ1, 8, 0)
    for bad in good:
        p = {k: (host if k == bad else t).data_ptr() for k, t in good.items()}
        side = rw.GfRwSide(p["d_text"], len(texts[0]), p["d_nl_pos"], int(nl.numel()), p["d_bases"], p["d_quals"], p["d_off"],
                           p["d_pre_bases"], p["d_pre_off"], p["d_out_text"], cap, p["d_out_off"])
        rc = L.gf_rw_format_device(h, C.addressof(settings), C.addressof(side), None, n, p["ws"], ws_bytes, p["totals"], None)
        assert rc == _lib.GF_ERR_NO_DEVICE and b"no CPU fallback" in L.gf_rw_last_error(), bad
    torch.cuda.synchronize()
    assert totals.cpu().tolist() == [0] * rw.TOTALS and out_off.cpu().tolist() == [0] * (n + 1)


# ---- every streamed route ---------------------------------------------------------------------------------------------------

CHUNK = 20_000
LENGTH, SKIP = 8, 2


def _records(path):
    lines = open(path, "rb").read().split(b"\n")
    return [lines[k:k + 4] for k in range(0, len(lines) - (len(lines) % 4), 4)]


def _write(path, records, final_newline):
    with open(path, "wb") as f:
        f.write(b"\n".join(b"\n".join(r) for r in records) + (b"\n" if final_newline else b""))


@pytest.fixture(scope="module")
def files(tmp_path_factory, gpu_device):
    """The three pairs of tests/golden/R1.fq / R2.fq and, so that the scans have matches, the planted pairs of
    tests.test_adapter_trim_gpu._trimmed_files, as the duplicate removal's route tests build their input — here as
    molecules: every mate carries an inline UMI of 8 bases and a spacer of 2; every fourth pair comes a second time
    under another UMI (" molB": a second molecule), every third a third time under the first one, in the other case
    (" copy": a PCR copy, which the removal drops), and two pairs are too short for the UMI.  With them, what the five
    steps leave, from their models, and the text the writer owes."""
    from tests.adapter_trim_model import trim_batch
    from tests.read_filter_model import filter_batch
    from tests.test_adapter_trim_gpu import ROUTE_SETTINGS, _trimmed_files
    tmp = tmp_path_factory.mktemp("read_write_routes")
    f = _trimmed_files(tmp)
    golden = os.path.join(ROOT, "tests", "golden")
    base = [_records(os.path.join(golden, "R1.fq")) + _records(f["r1"]),
            _records(os.path.join(golden, "R2.fq")) + _records(f["r2"])]
    n = len(base[0])
    assert n == len(base[1]) == 153
    rng = np.random.default_rng(78)
    umis = [(random_bases(rng, LENGTH), random_bases(rng, LENGTH)) for _ in range(n)]
    order = [(k, "A") for k in range(n)] + [(k, "molB") for k in range(0, n, 4)] + [(k, "copy") for k in range(0, n, 3)]
    order += [(1, "short"), (2, "short")]
    sides = [[], []]
    for at, (k, kind) in enumerate(order):
        u = umis[k]
        if kind == "molB":
            u = (u[0][::-1] + b"", u[1][:-1] + (b"A" if u[1][-1:] not in b"Aa" else b"C"))
        lower = kind == "copy"
        for side in (0, 1):
            name, seq, plus, qual = base[side][k]
            tag = b"" if kind == "A" else b" " + kind.encode()
            prefix = (u[side].swapcase() if lower else u[side]) + b"TG"
            if kind == "short" and side == k - 1:
                sides[side].append([name + tag, prefix[:7], plus, b"I" * 7])
            else:
                sides[side].append([name + tag, prefix + (seq.swapcase() if lower else seq), plus, b"I" * 10 + qual])
    for key, side, nl in (("w1", sides[0], True), ("w2", sides[1], False)):
        f[key] = str(tmp / (key + ".fq"))
        _write(f[key], side, nl)
    f["order"], f["texts"] = order, [open(f[key], "rb").read() for key in ("w1", "w2")]
    two = tmp / "two.txt"
    two.write_text("%s\n%s\n" % (f["csvs"][3], f["csvs"][0]))
    f["two"] = str(two)
    originals = [[(r[1], r[3]) for r in side] for side in sides]
    for pairs in (True, False):
        recs = list(zip(*originals)) if pairs else list(originals[0])
        cut = umi_model.cut(model.PER_READ if pairs else model.READ1, LENGTH, SKIP, recs)
        lists = [[r[s] for r in cut.records] for s in (0, 1)] if pairs else [cut.records]
        trimmed = trim_batch(lists[0], lists[1] if pairs else None, ROUTE_SETTINGS)
        kept = filter_batch(trimmed.reads[0], trimmed.reads[1] if pairs else None, f["fs"])
        cleaned = list(zip(*kept.reads)) if pairs else list(kept.reads[0])
        keys = umi_model.dedup_keys(cleaned, cut.codes)
        table = dedup_model.Table()
        table.insert(keys, 0)
        dup = table.duplicates(keys, 0)
        finals = [[(b"", b"") if d else r for r, d in zip(side, dup)] for side in kept.reads]
        source = model.PER_READ if pairs else model.READ1
        texts = f["texts"] if pairs else f["texts"][:1]
        pre = originals if pairs else originals[:1]
        f["want_pairs" if pairs else "want_single"] = {
            "plain": model.format_reads(texts, finals), "tagged": model.format_reads(texts, finals, source, LENGTH, pre),
            "dup": dup}
    return f


def _all_steps(f, single=False):
    """All five steps, each a fresh object."""
    from genefuserust_amd.read_filter import ReadFilter
    from genefuserust_amd.read_qc import ReadQc
    from tests.test_adapter_trim_gpu import _route_config
    return dict(umi=Umi("read1" if single else "per_read", LENGTH, SKIP), adapter_trim=_route_config(),
                read_filter=ReadFilter(*f["fs"]), dedup=dd.Dedup(slots=1024), qc=ReadQc())


def _texts(results):
    from genefuserust_amd import report_json, report_text
    return report_text(results), report_json(results, "cmd", "v", "t")


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


@pytest.mark.gpu
def test_pair_route_writes_the_models_text_whatever_the_chunks(files, tmp_path):
    from genefuserust_amd.scan import scan_pair_end_report
    f = files
    want = f["want_pairs"]
    assert want["plain"].totals[0] > 100 and want["plain"].totals[4] > 40 and sum(want["dup"]) > 20
    args = (f["fa"], f["csvs"][3], f["w1"], f["w2"])
    plain = scan_pair_end_report(*args, chunk_bytes=CHUNK, **_all_steps(f))
    assert plain[1]["chunks"] >= 3 and len(plain[0]) > 0
    outs = {}
    for name, chunk_bytes in (("one", 1 << 22), ("many", CHUNK)):
        w = ReadWriter(str(tmp_path / (name + "_1.fq")), str(tmp_path / (name + "_2.fq")))
        got = scan_pair_end_report(*args, chunk_bytes=chunk_bytes, **_all_steps(f), write_reads=w)
        assert got[1]["chunks"] == (1 if name == "one" else plain[1]["chunks"])
        outs[name] = (_read(w.out1), _read(w.out2))
        assert not os.path.exists(w.out1 + ".tmp") and not os.path.exists(w.out2 + ".tmp")
        # the counters are the model's, behind the duplicate removal's; everything else is the scan's without the writer
        assert {k: got[1][k] for k in rw.WRITE_COUNTER_KEYS} == model.counters(want["plain"].totals)
        keys = list(got[1])
        at = keys.index("dedup_bases_removed")
        assert tuple(keys[at + 1:at + 4]) == rw.WRITE_COUNTER_KEYS
        rest = {k: v for k, v in got[1].items() if k not in rw.WRITE_COUNTER_KEYS}
        if name == "many":
            assert rest == plain[1] and list(rest) == list(plain[1])
        assert _texts(got[0]) == _texts(plain[0])
        r = w.result()
        assert (r.records, r.bases, r.bytes, r.not_written) == (
            want["plain"].totals[0], want["plain"].totals[1], tuple(want["plain"].totals[2:4]), want["plain"].totals[4])
    assert outs["one"] == outs["many"] == tuple(want["plain"].texts)
    assert b" copy" not in outs["one"][0] and b" molB" in outs["one"][0] and b" short" not in outs["one"][1]
    # R1 and R2 stay in step
    names = [[line.split(b" ")[0] for line in text.split(b"\n")[0::4] if line] for text in outs["one"]]
    assert len(names[0]) == len(names[1]) == want["plain"].totals[0]


@pytest.mark.gpu
def test_gz_output_gunzips_to_the_plain_output_and_tags_go_into_the_names(files, tmp_path):
    from genefuserust_amd.scan import scan_pair_end_files
    f = files
    want = f["want_pairs"]
    args = (f["fa"], f["csvs"][3], f["w1"], f["w2"])
    w = ReadWriter(str(tmp_path / "o1.fq.gz"), str(tmp_path / "o2.fq.gz"), umi_in_name=True, compress_level=6)
    got = scan_pair_end_files(*args, chunk_bytes=CHUNK, **_all_steps(f), write_reads=w)
    assert got[1]["chunks"] >= 3
    texts = (gzip.decompress(_read(w.out1)), gzip.decompress(_read(w.out2)))
    assert texts == tuple(want["tagged"].texts)
    assert _read(w.out1)[:2] == b"\x1f\x8b" and len(_read(w.out1)) < len(texts[0])
    assert got[1]["written_bytes"] == len(texts[0]) + len(texts[1]) == sum(want["tagged"].totals[2:4])
    # both mates of a pair carry the same tag
    tags = [[line.split(b" ")[0].rsplit(b":", 1)[1] for line in t.split(b"\n")[0::4] if line] for t in texts]
    assert tags[0] == tags[1] and all(len(t) == 2 * LENGTH + 1 and t[LENGTH:LENGTH + 1] == b"_" for t in tags[0])


@pytest.mark.gpu
def test_two_csvs_write_once_and_single_end_writes_r1(files, tmp_path):
    from genefuserust_amd.multi_csv_scan import scan_multi_csv_report
    from genefuserust_amd.scan import scan_single_end_files
    f = files
    w = ReadWriter(str(tmp_path / "m1.fq"), str(tmp_path / "m2.fq"))
    got = scan_multi_csv_report(f["fa"], f["two"], f["w1"], f["w2"], chunk_bytes=CHUNK, **_all_steps(f), write_reads=w)
    plain = scan_multi_csv_report(f["fa"], f["two"], f["w1"], f["w2"], chunk_bytes=CHUNK, **_all_steps(f))
    assert len(got) == 2 and (_read(w.out1), _read(w.out2)) == tuple(f["want_pairs"]["plain"].texts)
    for (_, results, counters), (_, plain_results, plain_counters) in zip(got, plain):
        assert {k: counters.pop(k) for k in rw.WRITE_COUNTER_KEYS} == model.counters(f["want_pairs"]["plain"].totals)
        assert counters == plain_counters and _texts(results) == _texts(plain_results)
    want = f["want_single"]
    assert want["plain"].totals[0] > 100 and want["plain"].totals[4] > 20
    for tagged in (False, True):
        w = ReadWriter(str(tmp_path / ("s%d.fq" % tagged)), umi_in_name=tagged)
        got = scan_single_end_files(f["fa"], f["csvs"][3], f["w1"], chunk_bytes=CHUNK, **_all_steps(f, single=True),
                                    write_reads=w)
        key = "tagged" if tagged else "plain"
        assert _read(w.out1) == want[key].texts[0] and got[1]["chunks"] >= 3
        assert {k: got[1][k] for k in rw.WRITE_COUNTER_KEYS} == model.counters(want[key].totals)
    plain = scan_single_end_files(f["fa"], f["csvs"][3], f["w1"], chunk_bytes=CHUNK, **_all_steps(f, single=True))
    assert {k: v for k, v in got[1].items() if k not in rw.WRITE_COUNTER_KEYS} == plain[1] and got[0] == plain[0]


@pytest.mark.gpu
def test_the_writer_alone_rewrites_the_records_with_bases(files, tmp_path):
    """``write_reads`` with no other step: the text as it came, but for the pair with a mate of no bases — none here,
    so but for the final newline R2's file lacks."""
    from genefuserust_amd.scan import scan_pair_end_files
    f = files
    w = ReadWriter(str(tmp_path / "a1.fq"), str(tmp_path / "a2.fq"))
    got = scan_pair_end_files(f["fa"], f["csvs"][3], f["w1"], f["w2"], chunk_bytes=CHUNK, write_reads=w)
    plain = scan_pair_end_files(f["fa"], f["csvs"][3], f["w1"], f["w2"], chunk_bytes=CHUNK)
    assert (_read(w.out1), _read(w.out2)) == (f["texts"][0], f["texts"][1] + b"\n")
    assert got[0] == plain[0] and {k: v for k, v in got[1].items() if k not in rw.WRITE_COUNTER_KEYS} == plain[1]
    assert got[1]["written_records"] == len(f["order"]) == got[1]["pairs"]


# ---- round trip -------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_round_trip(files, tmp_path):
    """The written files scanned with no preparation step report what the first scan reported, under the sequencer's
    names; written with ``umi_in_name``, a second run that reads the UMIs from the names tags every record and finds no
    duplicate left."""
    from genefuserust_amd import report_text
    from genefuserust_amd.scan import scan_pair_end_files, scan_pair_end_report
    f = files
    args = (f["fa"], f["csvs"][3])
    w = ReadWriter(str(tmp_path / "c1.fq"), str(tmp_path / "c2.fq.gz"))
    first = scan_pair_end_report(*args, f["w1"], f["w2"], chunk_bytes=CHUNK, **_all_steps(f), write_reads=w)
    again = scan_pair_end_report(*args, w.out1, w.out2)
    assert report_text(again[0]) == report_text(first[0]) and len(first[0]) > 0
    assert again[1]["pairs"] == first[1]["written_records"]
    sequencer = {r[0] for r in _records(f["w1"])}
    assert all(line in sequencer for line in _read(w.out1).split(b"\n")[0::4] if line)
    w = ReadWriter(str(tmp_path / "t1.fq"), str(tmp_path / "t2.fq"), umi_in_name=True)
    first = scan_pair_end_files(*args, f["w1"], f["w2"], chunk_bytes=CHUNK, **_all_steps(f), write_reads=w)
    second = scan_pair_end_files(*args, w.out1, w.out2, umi=Umi("name"), dedup=dd.Dedup(slots=1024))
    assert second[1]["pairs"] == first[1]["written_records"] == second[1]["umi_reads_tagged"] > 100
    assert second[1]["umi_missing"] == 0 and second[1]["dedup_duplicates"] == 0
    assert second[1]["dedup_unique"] == second[1]["pairs"]
