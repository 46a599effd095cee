"""libgfumi.so on the device (include/gf_umi.h): the inline cut, the name parser and the key mixing against the model
(tests/umi_model.py) — every array compared exactly —, the duplicate removal with UMI codes, and every route of a scan
with ``umi``: whole file against streamed, both against the model over the files."""
import ctypes as C
import re

import numpy as np
import pytest

from genefuserust_amd import dedup as dd
from genefuserust_amd import umi as um
from genefuserust_amd.umi import Umi
from tests import dedup_model
from tests import umi_model as model
from tests.umi_cases import GRID, NAME_CASES, fastq_text, random_bases, record, records_for

SIZES = [0, 1, 255, 256, 257, 600]
SOURCE_NAMES = {model.READ1: "read1", model.READ2: "read2", model.PER_READ: "per_read"}


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


def _u64(t):
    return [int(x) for x in t.cpu().numpy().view(np.uint64)]


def _i64(values):
    import torch
    return torch.from_numpy(np.asarray(values, dtype=np.uint64).view(np.int64).copy()).cuda()


def _batch(records, lead: int = 0):
    """The records ((bases, quals) each) as the full FASTQ cut leaves them; ``lead`` bytes of another record in front of
    the first, so that the first byte lies at that alignment and the offsets do not start at 0."""
    import torch
    from genefuserust_amd.fastq import FastqBatch
    off = lead + np.concatenate([[0], np.cumsum([len(b) for b, _ in records], dtype=np.int64)]).astype(np.int64)
    none = torch.zeros(0, dtype=torch.int64, device="cuda")
    return FastqBatch(_up(b"G" * lead + b"".join(b for b, _ in records)),
                      _up(b"~" * lead + b"".join(q for _, q in records)), torch.from_numpy(off).cuda(), len(records),
                      none, 0, 0)


def _records_of(batch):
    off = batch.offsets.cpu().numpy()
    b, q = batch.bases.cpu().numpy().tobytes(), batch.quals.cpu().numpy().tobytes()
    assert off[0] == 0 and batch.qual_off is None
    return [(b[s:e], q[s:e]) for s, e in zip(off, off[1:])]


def _cut_against_the_model(ix, source, length, skip, records, leads):
    """One ``cut_umis_device`` call over reads or pairs: records, codes and totals are the model's."""
    pairs = bool(records) and isinstance(records[0][0], tuple)
    sides = [[r[0] for r in records], [r[1] for r in records]] if pairs else [records]
    batches = [_batch(side, lead) for side, lead in zip(sides, leads)]
    *out, codes, totals = um.cut_umis_device(ix, Umi(SOURCE_NAMES[source], length, skip), *batches)
    want = model.cut(source, length, skip, records)
    assert len(out) == len(sides) and _u64(codes) == want.codes
    assert totals.cpu().tolist() == want.totals
    got = [_records_of(b) for b in out]
    assert (list(zip(*got)) if pairs else got[0]) == want.records
    return want


# ---- the inline cut -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_cut_batch_sizes(ix, n):
    """Every batch size around the tile, every record length of the cases (0, c - 1, c, c + 1, 15, 16, 17, 150, 151,
    5000), pairs whose mates are out of step, then reads; offsets that do not start at 0."""
    rng = np.random.default_rng(100 + n)
    want = _cut_against_the_model(ix, model.PER_READ, 8, 2, records_for(rng, n, 10, True), (n % 16 + 1, (n + 7) % 16))
    assert want.totals[0] == n and want.totals[1] + want.totals[5] == n
    if n >= 255:
        assert want.totals[3] > 0 and want.totals[5] > 20 and want.totals[6] > 5000 and want.totals[4] == 20 * want.totals[1]
    single = _cut_against_the_model(ix, model.READ1, 8, 2, records_for(rng, n, 10, False), ((5 * n) % 16,))
    assert single.totals[4] == 10 * single.totals[1]
    _cut_against_the_model(ix, model.PER_READ, 8, 2, records_for(rng, n, 10, False), (3,))     # per_read is read1 there


@pytest.mark.gpu
def test_cut_every_lead_and_every_source(ix):
    """Every lead 0 .. 15 of the first byte, both sides at different leads, each inline source on pairs and reads."""
    rng = np.random.default_rng(7)
    emptied = 0
    for lead in range(16):
        for source in (model.READ1, model.READ2, model.PER_READ):
            want = _cut_against_the_model(ix, source, 8, 2, records_for(rng, 23, 10, True), (lead, (3 * lead + 5) % 16))
            emptied += want.totals[5]
        for source in (model.READ1, model.PER_READ):
            _cut_against_the_model(ix, source, 8, 2, records_for(rng, 23, 10, False), (lead,))
    assert emptied > 100


@pytest.mark.gpu
def test_cut_every_length_and_skip_of_the_grid(ix):
    rng = np.random.default_rng(9)
    for k, (length, skip) in enumerate(GRID):
        source = (model.READ1, model.READ2, model.PER_READ)[k % 3]
        want = _cut_against_the_model(ix, source, length, skip, records_for(rng, 40, length + skip, True),
                                      (k % 16, (k + 9) % 16))
        assert want.totals[1] > 0 and want.totals[5] > 0


@pytest.mark.gpu
def test_cut_a_mate_emptied_by_the_other_sides_short_record(ix):
    q = b"I" * 200
    long, short = (b"ACGTACGTAC" + b"GATTACA" * 20, q[:150]), (b"ACGTACGTA", q[:9])
    exact = (b"acgtNcgtac", q[:10])
    pairs = [(long, long), (long, short), (short, long), (exact, long), (long, exact), ((b"", b""), long), (exact, exact),
             (short, short), ((b"", b""), (b"", b""))]
    per_read = _cut_against_the_model(ix, model.PER_READ, 8, 2, pairs, (4, 11))
    assert [int(bool(c)) for c in per_read.codes] == [1, 0, 0, 1, 1, 0, 1, 0, 0]
    assert per_read.records[1] == ((b"", b""), (b"", b"")) and per_read.records[3][0] == (b"", b"")
    assert per_read.records[6] == ((b"", b""), (b"", b"")) and per_read.codes[6] != 0      # cut to nothing, but tagged
    read1 = _cut_against_the_model(ix, model.READ1, 8, 2, pairs, (0, 15))
    assert [int(bool(c)) for c in read1.codes] == [1, 1, 0, 1, 1, 0, 1, 0, 0]
    assert read1.records[1][1] == short and read1.records[2] == ((b"", b""), (b"", b""))   # R2 passes; R2 emptied by R1
    read2 = _cut_against_the_model(ix, model.READ2, 8, 2, pairs, (9, 2))
    assert [int(bool(c)) for c in read2.codes] == [1, 0, 1, 1, 1, 1, 1, 0, 0]
    # the code is the UMI's alone: the same UMI on other bases, in the other case
    a = _cut_against_the_model(ix, model.READ1, 8, 2, [(b"ACGTACGTNN" + b"A" * 30, q[:40])], (1,))
    b = _cut_against_the_model(ix, model.READ1, 8, 2, [(b"acgtacgtGG" + b"C" * 50, q[:60])], (6,))
    assert a.codes == b.codes == [0x1d189c7f508326f9] and a.totals[3] == 0
    p = _cut_against_the_model(ix, model.PER_READ, 4, 0, [((b"ACGTAA", q[:6]), (b"TTGACC", q[:6]))], (2, 3))
    assert p.codes == [0x8a0ec19742ea7304]


@pytest.mark.gpu
def test_cut_writes_nothing_outside_its_outputs_and_leaves_its_inputs(ix):
    """The raw call with every buffer inside junk: the inputs and the junk around them stay, the outputs hold the
    model's bytes, and the bytes behind them stay."""
    import torch
    rng = np.random.default_rng(3)
    records = records_for(rng, 300, 10, True)
    want = model.cut(model.PER_READ, 8, 2, records)
    n, guard = len(records), 64
    ins, outs, ptrs, out_ptrs = [], [], [], []
    for side, lead in ((0, 5), (1, 12)):
        recs = [r[side] for r in records]
        total = sum(len(b) for b, _ in recs)
        off = lead + guard + np.concatenate([[0], np.cumsum([len(b) for b, _ in recs])]).astype(np.int64)
        bases = _up(bytes(rng.integers(0, 256, guard + lead, dtype=np.uint8)) + b"".join(b for b, _ in recs) +
                    bytes(rng.integers(0, 256, guard, dtype=np.uint8)))
        quals = _up(bytes(rng.integers(0, 256, guard + lead, dtype=np.uint8)) + b"".join(q for _, q in recs) +
                    bytes(rng.integers(0, 256, guard, dtype=np.uint8)))
        d_off = torch.from_numpy(off).cuda()
        ins.append((bases, quals, d_off, bases.clone(), quals.clone(), d_off.clone()))
        ptrs += [bases.data_ptr(), quals.data_ptr(), d_off.data_ptr()]
        kept = sum(len(r[side][0]) for r in want.records)
        ob = torch.full((total + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        oq = torch.full((total + guard,), 0x5A, dtype=torch.uint8, device="cuda")
        oo = torch.full((n + 1 + 8,), -77, dtype=torch.int64, device="cuda")
        outs.append((ob, oq, oo, kept))
        out_ptrs += [ob.data_ptr(), oq.data_ptr(), oo.data_ptr()]
    L = um.lib()
    ws_bytes = int(L.gf_um_workspace_bytes(n))
    ws = torch.full((ws_bytes + guard,), 0x3C, dtype=torch.uint8, device="cuda")
    codes = torch.full((n + 8,), -5, dtype=torch.int64, device="cuda")
    totals = torch.tensor([1000, 0, 0, 0, 0, 0, 5], dtype=torch.int64, device="cuda")
    settings = Umi("per_read", 8, 2).settings()
    um.check(L.gf_um_cut_device(ix._handle(), C.addressof(settings), *ptrs, n, ws.data_ptr(), ws_bytes, *out_ptrs,
                                codes.data_ptr(), totals.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for bases, quals, d_off, b0, q0, o0 in ins:
        assert torch.equal(bases, b0) and torch.equal(quals, q0) and torch.equal(d_off, o0)
    for side, (ob, oq, oo, kept) in enumerate(outs):
        off = oo.cpu().numpy()
        assert off[0] == 0 and off[n] == kept and (off[n + 1:] == -77).all()
        b, q = ob.cpu().numpy(), oq.cpu().numpy()
        assert (b[kept:] == 0xA5).all() and (q[kept:] == 0x5A).all()
        got = [(b[s:e].tobytes(), q[s:e].tobytes()) for s, e in zip(off, off[1:n + 1])]
        assert got == [r[side] for r in want.records]
    assert (ws.cpu().numpy()[ws_bytes:] == 0x3C).all()
    assert _u64(codes[:n]) == want.codes and (codes[n:].cpu().numpy() == -5).all()
    # the totals are added into
    assert totals.cpu().tolist() == [a + b for a, b in zip([1000, 0, 0, 0, 0, 0, 5], want.totals)]


# ---- the names ------------------------------------------------------------------------------------------------------------

def _names_against_the_model(ix, text: bytes, n: int):
    from genefuserust_amd.fastq import fastq_cut_device
    d_text = _up(text)
    batch = fastq_cut_device(ix, d_text)
    assert int(batch.n_newlines) == text.count(b"\n")
    before = d_text.clone()
    codes, totals = um.name_umis_device(ix, d_text, batch._replace(n_records=n))
    want_codes, want_totals = model.names(text, n)
    assert _u64(codes) == want_codes and totals.cpu().tolist() == want_totals
    assert (d_text == before).all()
    return want_codes, want_totals


@pytest.mark.gpu
def test_names_every_case(ix):
    """Every name case as a FASTQ text: record 0 at byte 0, with and without the final newline, records past the text;
    then the same with \\r\\n lines."""
    rng = np.random.default_rng(5)
    lines = [line for line, _ in NAME_CASES if not line.endswith(b"\r")]
    records = [record(rng, 20 + k) for k in range(len(lines))]
    n = len(lines)
    for final_newline in (True, False):
        text = fastq_text(lines, records, final_newline=final_newline)
        assert text.startswith(lines[0])
        codes, totals = _names_against_the_model(ix, text, n)
        assert [bool(c) for c in codes] == [has for line, has in NAME_CASES if not line.endswith(b"\r")]
        assert codes[1] == codes[3] == 0xdecfd2a34e770449 and totals[3] >= 1 and totals[1] + totals[2] == n
        past, totals = _names_against_the_model(ix, text, n + 3)
        assert past[n:] == [0, 0, 0] and past[:n] == codes and totals[2] == n + 3 - totals[1]
    crlf = fastq_text(lines, records, crlf=True)
    assert _names_against_the_model(ix, crlf, n)[0] == codes
    # a last record that is its name line alone, without a newline; an empty text
    tail = fastq_text(lines[:2], records[:2]) + b"@last:ACGT"
    assert _names_against_the_model(ix, tail, 3)[0][2] == model.code(b"ACGT")
    assert _names_against_the_model(ix, b"", 2) == ([0, 0], [2, 0, 2, 0, 0, 0, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_names_batch_sizes(ix, n):
    """Illumina-style names of 40 to 70 bytes, every fifth without a UMI, around the tile's size."""
    rng = np.random.default_rng(50 + n)
    lines = []
    for k in range(n):
        field = random_bases(rng, int(rng.integers(6, 13))) + (b"+" + random_bases(rng, 8) if k % 3 == 0 else b"")
        name = b"@A00%d:%d:HXXXXXXX:%d:%d:%d:%d" % (k % 7, 100 + k, 1 + k % 4, 1101 + k, 1000 * k + 7, 31 * k)
        lines.append(name + (b"" if k % 5 == 4 else b":" + field) + b" %d:N:0:ACGTACGT" % (1 + k % 2))
    records = [record(rng, 30 + k % 5) for k in range(n)]
    codes, totals = _names_against_the_model(ix, fastq_text(lines, records, final_newline=n % 2 == 0), n)
    # (a name without the field ends in the y coordinate: digits, no UMI)
    assert totals[0] == n and totals[2] == n // 5 and totals[1] == n - n // 5


# ---- the key mixing, and the duplicate removal with codes --------------------------------------------------------------------

@pytest.mark.gpu
def test_mix_keys(ix):
    M = (1 << 64) - 1
    K, U = 0xab0fcab10dd0c6f9, 0x1d189c7f508326f9
    keys = [0, K, K, 0, 1, M, K, 5] + [dedup_model.mix(k) | 1 for k in range(1, 600)]
    codes = [U, 0, U, 0, M, 1, 0x8a0ec19742ea7304, M] + [dedup_model.mix(k + 7000) * (k % 4 != 0) for k in range(1, 600)]
    for n in (0, 1, 8, 255, 256, 257, len(keys)):
        rec_keys = _i64(keys[:n])
        out = um.mix_keys_device(ix, rec_keys, _i64(codes[:n]))
        assert out is rec_keys and _u64(rec_keys) == [model.mix_key(k, u) for k, u in zip(keys[:n], codes[:n])]
    mixed = [model.mix_key(k, u) for k, u in zip(keys, codes)]
    assert mixed[0] == 0 and mixed[1] == K and mixed[3] == 0          # K == 0 and U == 0 pass through
    assert mixed[2] == 0xff1a16f0056acf7f and mixed[6] == 0xf6e69183b4f4f21c and mixed[2] != K


def _apply_with_codes(ix, d, pairs, codes, leads=(3, 8)):
    sides = [[p[0] for p in pairs], [p[1] for p in pairs]]
    (l, r), totals = d.apply(ix, *[_batch(side, lead) for side, lead in zip(sides, leads)], umi_codes=_i64(codes))
    return list(zip(_records_of(l), _records_of(r))), totals.cpu().tolist()


@pytest.mark.gpu
def test_dedup_with_codes_keeps_molecules_and_removes_copies(ix):
    """Two identical pairs with different UMIs both stay; identical pairs with the same UMI in the other case are one
    molecule, and the lower index stays; a pair without a UMI goes by its bases; the same when the table grows between
    two calls."""
    rng = np.random.default_rng(21)
    a, b = (record(rng, 120), record(rng, 100)), (record(rng, 90), record(rng, 90))
    lower = tuple((s[0].lower(), s[1]) for s in a)
    u1, u2, u1_lower = model.code_pair(b"ACGTACGT", b"TTGACCAA"), model.code_pair(b"ACGTACGA", b"TTGACCAA"), \
        model.code_pair(b"acgtacgt", b"ttgaccaa")
    assert u1 == u1_lower != u2
    pairs = [a, a, lower, a, b, b, a, b]
    codes = [u1, u2, u1_lower, u1, 0, 0, 0, u2]
    want_dup = [0, 0, 1, 1, 0, 1, 0, 0]
    none = ((b"", b""), (b"", b""))
    for slots, filler in ((1024, 0), (1024, 600)):
        d = dd.Dedup(slots=slots)
        out, totals = _apply_with_codes(ix, d, pairs, codes)
        assert out == [none if dup else p for p, dup in zip(pairs, want_dup)]
        assert totals[:4] == [8, 8, 5, 3]
        if filler:     # distinct pairs that take the table past half full: it is rehashed, and the keys are still found
            more = [(record(rng, 40), record(rng, 40)) for _ in range(filler)]
            _apply_with_codes(ix, d, more, [model.code(b"ACGT")] * filler)
            assert d.slots > slots
        # the same pairs again: every one a duplicate now, but a new molecule on the old bases
        again, totals = _apply_with_codes(ix, d, [a, a, lower, b], [u1, u2 ^ 1, u1, 0], leads=(11, 0))
        assert again == [none, a, none, none] and totals[:4] == [4, 4, 1, 3]
    # without codes the bases alone decide: today's outcome
    plain = dd.Dedup(slots=1024)
    sides = [[p[0] for p in pairs], [p[1] for p in pairs]]
    (l, r), totals = plain.apply(ix, *[_batch(side, 0) for side in sides])
    assert totals.cpu().tolist()[:4] == [8, 8, 2, 6]
    # the keys offered are the model's
    keys = dd.keys_device(ix, *[_batch(side, 0) for side in sides])
    um.mix_keys_device(ix, keys, _i64(codes))
    assert _u64(keys) == model.dedup_keys(pairs, codes)
    with pytest.raises(ValueError, match="UMI codes"):
        plain.apply(ix, *[_batch(side, 0) for side in sides], umi_codes=_i64(codes[:3]))


# ---- every route ----------------------------------------------------------------------------------------------------------

CHUNK = 20_000
LENGTH, SKIP = 8, 2


def _fastq_records(path):
    lines = open(path, "rb").read().split(b"\n")
    return [lines[k:k + 4] for k in range(0, len(lines) - (len(lines) % 4), 4)]


def _write(path, records, final_newline):
    with open(path, "wb") as f:
        f.write(b"\n".join(b"\n".join(r) for r in records) + (b"\n" if final_newline else b""))


@pytest.fixture(scope="module")
def files(tmp_path_factory, gpu_device):
    return _make_files(tmp_path_factory.mktemp("umi_routes"))


def _make_files(tmp):
    """The planted pairs of tests.test_adapter_trim_gpu._trimmed_files as molecules with UMIs: every pair once
    (molecule A); every fourth a second time with another UMI (" molB": a second molecule with the same bases); every
    third a third time with A's UMI, every other of those in lower case (" copy": a PCR copy); a few pairs too short
    for the UMI; a few names without one (both kinds with UMIs of their own, so that they are nobody's copies).  Inline
    files carry the UMI and a spacer in front of both mates, name files in
    R1's name.  The "u" files hold the molecules without the copies."""
    from tests.test_adapter_trim_gpu import _trimmed_files
    f = _trimmed_files(tmp)
    base = [_fastq_records(f["r1"]), _fastq_records(f["r2"])]
    n = len(base[0])
    assert n == len(base[1]) == 150
    rng = np.random.default_rng(77)
    umis = [(random_bases(rng, LENGTH).upper().replace(b"N", b"A"), random_bases(rng, LENGTH).upper().replace(b"N", b"C"))
            for _ in range(n)]
    umis[6] = (b"ACGNACGT", umis[6][1])
    order = [(k, "A") for k in range(n)] + [(k, "B") for k in range(0, n, 4)] + [(k, "copy") for k in range(0, n, 3)]
    order += [(k, "short") for k in (1, 2)] + [(k, "bare") for k in (5, 9, 13)]
    inline, named = [[], []], [[], []]
    for at, (k, kind) in enumerate(order):
        u = umis[k]
        if kind == "B":
            u = (u[0][::-1], u[1][:-1] + (b"A" if u[1][-1:] != b"A" else b"C"))
        elif kind in ("short", "bare"):
            u = (u[1], u[0])
        assert kind in ("A", "copy") or (u[0] != umis[k][0] and u[1] != umis[k][1])
        lower = kind == "copy" and at % 2 == 0
        for side in (0, 1):
            name, seq, plus, qual = base[side][k]
            tag = b"" if kind == "A" else b" " + (b"mol" if kind == "B" else b"") + kind.encode()
            prefix = (u[side].lower() if lower else u[side]) + b"TG"
            seq_out = seq.lower() if lower else seq
            if kind == "short":      # R1 (k == 1) or R2 (k == 2) shorter than the UMI and its spacer
                short = side == k - 1
                inline[side].append([name + tag, prefix[:7] if short else prefix + seq_out, plus,
                                     b"I" * 7 if short else b"I" * 10 + qual])
            else:
                inline[side].append([name + tag, prefix + seq_out, plus, b"I" * 10 + qual])
            field = b"" if kind == "bare" else b":" + u[0] + b"+" + u[1]
            field = field.lower() if lower else field
            # (the name's first token: the sequencer's name, then the UMI; the tag goes behind a space)
            named[side].append([name.split(b" ")[0] + field + tag, seq_out, plus, qual])
    f["order"] = order
    keep = [at for at, (_, kind) in enumerate(order) if kind != "copy"]
    for key, sides in (("i", inline), ("n", named)):
        for side, nl in ((0, True), (1, False)):
            f["%s%d" % (key, side + 1)] = str(tmp / ("%s%d.fq" % (key, side + 1)))
            f["u%s%d" % (key, side + 1)] = str(tmp / ("u%s%d.fq" % (key, side + 1)))
            _write(f["%s%d" % (key, side + 1)], sides[side], nl)
            _write(f["u%s%d" % (key, side + 1)], [sides[side][at] for at in keep], nl)
        f[key + "_sides"] = [[(r[1], r[3]) for r in side] for side in sides]
        f[key + "_text"] = open(f[key + "1"], "rb").read()
    two = tmp / "two.txt"
    two.write_text("%s\n%s\n" % (f["csvs"][3], f["csvs"][0]))
    f["two"] = str(two)
    return f


def _model_scan(f, key, source, length, skip, pairs=True):
    """What a scan with ``umi`` and ``dedup`` leaves, from the models: (the UMI step's five counters, the four dedup
    counters, the duplicate flags)."""
    sides = f[key + "_sides"]
    records = list(zip(*sides)) if pairs else list(sides[0])
    if source == model.NAME:
        codes, totals = model.names(f[key + "_text"], len(records))
        cut = records
    else:
        got = model.cut(source, length, skip, records)
        cut, codes, totals = got.records, got.codes, got.totals
    keys = model.dedup_keys(cut, codes)
    t = dedup_model.Table()
    dd_totals = t.insert(keys, 0)
    dup = t.duplicates(keys, 0)
    removed = sum(len(r[0][0]) + len(r[1][0]) if pairs else len(r[0]) for r, d in zip(cut, dup) if d)
    return (dict(zip(um.UMI_COUNTER_KEYS, (totals[1], totals[2], totals[3], totals[4], totals[5]))),
            dict(zip(dd.DEDUP_COUNTER_KEYS, (dd_totals[1], dd_totals[2], sum(dup), removed))), dup)


def _texts(results):
    from genefuserust_amd import report_json, report_text
    return report_text(results), report_json(results, "cmd", "v", "t")


@pytest.mark.gpu
@pytest.mark.parametrize("source,key", [("per_read", "i"), ("read1", "i"), ("read2", "i"), ("name", "n")])
def test_pair_routes_whole_file_and_streamed(files, source, key):
    from genefuserust_amd.scan import scan_pair_end_files, scan_pair_end_report
    f = files
    u = Umi(source, *((LENGTH, SKIP) if source != "name" else ()))
    args = (f["fa"], f["csvs"][3], f[key + "1"], f[key + "2"])
    want_umi, want_dd, dup = _model_scan(f, key, model.SOURCES[source], u.length, u.skip)
    kinds = [kind for _, kind in f["order"]]
    if source in ("per_read", "name"):
        # the copies are removed, the second molecules stay
        assert [bool(d) for d in dup] == [kind == "copy" for kind in kinds]
        assert want_umi["umi_with_n"] == 2      # molecule A of pair 6, and its copy
    assert want_umi["umi_too_short"] == (0 if source == "name" else 2 if source == "per_read" else 1)
    assert want_umi["umi_missing"] == (3 if source == "name" else 0)
    whole, streamed = dd.Dedup(slots=1024), dd.Dedup(slots=1024)
    got = scan_pair_end_files(*args, dedup=whole, umi=u)
    got_streamed = scan_pair_end_files(*args, dedup=streamed, umi=u, chunk_bytes=CHUNK)
    assert got_streamed[1].pop("chunks") >= 4
    assert got == got_streamed and whole.result() == streamed.result()
    assert {k: got[1][k] for k in um.UMI_COUNTER_KEYS} == want_umi
    assert {k: got[1][k] for k in dd.DEDUP_COUNTER_KEYS} == want_dd
    keys = list(got[1])
    at = keys.index("umi_reads_tagged")
    assert tuple(keys[at:at + 10]) == um.UMI_COUNTER_KEYS + dd.DEDUP_COUNTER_KEYS + ("complexity",)
    names = [m.m_name for m in got[0]]
    if source in ("per_read", "name"):
        # the matches are those of the molecules alone, scanned without the removal: both molecules of a pair, no copy
        alone = scan_pair_end_files(f["fa"], f["csvs"][3], f["u%s1" % key], f["u%s2" % key], umi=u)
        assert sorted(names) == sorted(m.m_name for m in alone[0]) and len(names) > 0
        assert any(b" molB" in nm for nm in names) and not any(b" copy" in nm for nm in names)
        assert {k: alone[1][k] for k in ("umi_missing", "umi_too_short")} == \
            {k: want_umi[k] for k in ("umi_missing", "umi_too_short")}
        assert alone[1]["umi_reads_tagged"] == want_umi["umi_reads_tagged"] - kinds.count("copy")
    # text and JSON of the report are equal across the routes
    reports = [scan_pair_end_report(*args, dedup=dd.Dedup(slots=1024), umi=u, **kw)
               for kw in ({}, {"chunk_bytes": CHUNK})]
    reports[1][1].pop("chunks")
    assert reports[0][1] == reports[1][1] and _texts(reports[0][0]) == _texts(reports[1][0]) and len(reports[0][0]) > 0


@pytest.mark.gpu
def test_umi_alone_cuts_or_counts_and_none_is_todays_scan(files):
    """``umi`` without ``dedup``: an inline source cuts — the scan is that of the files without the UMIs, the name files
    —, the name source only counts.  ``umi=None`` with ``dedup``: the bases alone decide, and the second molecules go."""
    from genefuserust_amd.scan import scan_pair_end_files
    f = files
    plain = scan_pair_end_files(f["fa"], f["csvs"][3], f["n1"], f["n2"])
    for kw in ({}, {"chunk_bytes": CHUNK}):
        cut = scan_pair_end_files(f["fa"], f["csvs"][3], f["i1"], f["i2"], umi=Umi("per_read", LENGTH, SKIP), **kw)
        counted = scan_pair_end_files(f["fa"], f["csvs"][3], f["n1"], f["n2"], umi=Umi(), **kw)
        for got in (cut, counted):
            got[1].pop("chunks", None)
        assert {k: v for k, v in counted[1].items() if k not in um.UMI_COUNTER_KEYS} == plain[1]
        assert counted[0] == plain[0] and counted[1]["umi_missing"] == 3 and counted[1]["umi_bases_cut"] == 0
        # the two pairs too short for the UMI are scanned as empty reads; nothing else differs from the name files' scan
        assert cut[1]["umi_too_short"] == 2 and cut[1]["umi_bases_cut"] == 20 * cut[1]["umi_reads_tagged"]
        assert cut[1]["pairs"] == plain[1]["pairs"] and len(cut[0]) > 0
        assert sorted(m.m_name for m in cut[0]) == \
            sorted(re.sub(rb":[A-Za-z+]+", b"", m.m_name) for m in plain[0] if b" short" not in m.m_name)
    by_bases = scan_pair_end_files(f["fa"], f["csvs"][3], f["n1"], f["n2"], dedup=dd.Dedup(slots=1024))
    assert not any(b" molB" in m.m_name or b" copy" in m.m_name for m in by_bases[0]) and len(by_bases[0]) > 0
    assert "umi_reads_tagged" not in by_bases[1] and by_bases[1]["dedup_duplicates"] > 80


@pytest.mark.gpu
def test_qc_with_umi_alone_measures_the_same_stages_whole_file_and_streamed(files):
    """``qc`` and ``umi`` with no other step: the name source moves no byte, so neither route measures "after" and the
    document shows "before" twice; an inline source cuts, so both measure it, on the cut records.  The documents of the
    two routes are equal either way."""
    from genefuserust_amd.read_qc import ReadQc, report_json
    from genefuserust_amd.scan import scan_pair_end_files
    f = files
    for u, key in ((Umi(), "n"), (Umi("per_read", LENGTH, SKIP), "i")):
        docs, qcs = [], []
        for kw in ({}, {"chunk_bytes": CHUNK}):
            qc = ReadQc()
            got = scan_pair_end_files(f["fa"], f["csvs"][3], f[key + "1"], f[key + "2"], qc=qc, umi=u, **kw)
            got[1].pop("chunks", None)
            docs.append(report_json(qc.result(), got[1], None, u))
            qcs.append(qc)
        assert docs[0] == docs[1]
        assert [("after" in qc._stages) for qc in qcs] == [u.inline] * 2
        r = qcs[1].result()
        before, after = r.summary("before"), r.summary("after")
        assert before["total_reads"] == 2 * len(f["order"])
        if u.inline:
            want_umi = _model_scan(f, key, model.PER_READ, LENGTH, SKIP)[0]
            removed = model.cut(model.PER_READ, LENGTH, SKIP, list(zip(*f[key + "_sides"]))).totals[6]
            assert before["total_bases"] - after["total_bases"] == want_umi["umi_bases_cut"] + removed > 0
        else:
            assert after == before


@pytest.mark.gpu
def test_host_memory_behind_any_pointer_is_refused(ix):
    """Not only the first pointers of a call: a host array where the kernel would read or write is ``GF_ERR_NO_DEVICE``,
    and nothing is launched."""
    import torch
    from genefuserust_amd import _lib
    rng = np.random.default_rng(2)
    b = _batch([record(rng, 40) for _ in range(5)])
    text = _up(fastq_text([b"@r%d:ACGT" % i for i in range(5)], [(b"ACGT", b"FFFF")] * 5))
    from genefuserust_amd.fastq import fastq_cut_device
    cut = fastq_cut_device(ix, text)
    L, h = um.lib(), ix._handle()
    codes = torch.zeros(5, dtype=torch.int64, device="cuda")
    totals = torch.zeros(um.TOTALS, dtype=torch.int64, device="cuda")
    host = torch.zeros(64, dtype=torch.int64)
    # the names call: device text and totals, the newline positions or the codes on the host
    for nl, out in ((host, codes), (cut.nl_pos, host)):
        rc = L.gf_um_names_device(h, text.data_ptr(), text.numel(), nl.data_ptr(), int(cut.n_newlines), 5,
                                  out.data_ptr(), totals.data_ptr(), None)
        assert rc == _lib.GF_ERR_NO_DEVICE and b"no CPU fallback" in L.gf_um_last_error()
    # the cut: every pointer but one on the device
    ws_bytes = int(L.gf_um_workspace_bytes(5))
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
    outs = [torch.zeros(256, dtype=torch.uint8, device="cuda") for _ in range(2)]
    out_off = torch.zeros(6, dtype=torch.int64, device="cuda")
    settings = Umi("read1", 8).settings()
    good = dict(bases=b.bases, quals=b.quals, ws=ws, out_bases=outs[0], out_quals=outs[1], out_off=out_off, codes=codes)
    for bad in good:
        p = {k: (host if k == bad else t).data_ptr() for k, t in good.items()}
        rc = L.gf_um_cut_device(h, C.addressof(settings), p["bases"], p["quals"], b.offsets.data_ptr(), None, None, None,
                                5, p["ws"], ws_bytes, p["out_bases"], p["out_quals"], p["out_off"], None, None, None,
                                p["codes"], totals.data_ptr(), None)
        assert rc == _lib.GF_ERR_NO_DEVICE and b"no CPU fallback" in L.gf_um_last_error(), bad
    torch.cuda.synchronize()
    assert totals.cpu().tolist() == [0] * um.TOTALS and codes.cpu().tolist() == [0] * 5


@pytest.mark.gpu
def test_single_end_routes(files):
    from genefuserust_amd.scan import scan_single_end_files
    f = files
    for source, key in (("read1", "i"), ("name", "n"), ("per_read", "i")):
        u = Umi(source, *((LENGTH, SKIP) if source != "name" else ()))
        want_umi, want_dd, dup = _model_scan(f, key, model.READ1 if source == "per_read" else model.SOURCES[source],
                                             u.length, u.skip, pairs=False)
        assert 40 < sum(dup) < 60
        results = []
        for kwargs in (dict(route="device"), dict(route="host"), dict(chunk_bytes=CHUNK)):
            d = dd.Dedup(slots=1024)
            got = scan_single_end_files(f["fa"], f["csvs"][3], f[key + "1"], **kwargs, dedup=d, umi=u)
            got[1].pop("chunks", None)
            got[1].pop("retried_reads", None)   # (the host route does not count them)
            assert {k: got[1][k] for k in um.UMI_COUNTER_KEYS} == want_umi
            assert {k: got[1][k] for k in dd.DEDUP_COUNTER_KEYS} == want_dd
            results.append(got)
        assert results[0] == results[1] == results[2]
    with pytest.raises(ValueError, match="read2"):
        scan_single_end_files(f["fa"], f["csvs"][3], f["i1"], umi=Umi("read2", LENGTH, SKIP))


@pytest.mark.gpu
def test_two_csvs_are_tagged_once(files):
    from genefuserust_amd.multi_csv_scan import scan_multi_csv_report
    from genefuserust_amd.scan import scan_pair_end_report
    f = files
    u = Umi("per_read", LENGTH, SKIP)
    want_umi, want_dd, _ = _model_scan(f, "i", model.PER_READ, LENGTH, SKIP)
    outs = []
    for chunk_bytes in (CHUNK, None):
        d = dd.Dedup(slots=1024)
        got = scan_multi_csv_report(f["fa"], f["two"], f["i1"], f["i2"], chunk_bytes=chunk_bytes, dedup=d, umi=u)
        assert len(got) == 2 and d.offered == len(f["order"])
        for _, _, counters in got:
            counters.pop("chunks", None)
            assert {k: counters[k] for k in um.UMI_COUNTER_KEYS} == want_umi
            assert {k: counters[k] for k in dd.DEDUP_COUNTER_KEYS} == want_dd
        outs.append(got)
    assert outs[0] == outs[1]
    one = scan_pair_end_report(f["fa"], f["csvs"][3], f["i1"], f["i2"], dedup=dd.Dedup(slots=1024), umi=u)
    assert _texts(outs[0][0][1]) == _texts(one[0]) and outs[0][0][2] == one[1] and len(one[0]) > 0


@pytest.mark.gpu
def test_a_lean_cut_and_a_wrong_source_are_refused(ix):
    rng = np.random.default_rng(1)
    b = _batch([record(rng, 40) for _ in range(5)])
    with pytest.raises(ValueError, match="full FASTQ cut"):
        um.cut_umis_device(ix, Umi("read1", 8), b._replace(qual_off=b.offsets))
    with pytest.raises(ValueError, match="inline source"):
        um.cut_umis_device(ix, Umi(), b)
    with pytest.raises(ValueError, match="read2"):
        um.cut_umis_device(ix, Umi("read2", 8), b)
