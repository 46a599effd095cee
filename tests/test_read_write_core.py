"""The arithmetic of libgfwrite.so on the host: genefuserust_amd/scan_csrc/gf_rw_core.h, the very text the kernels run,
compiled with g++ under AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone program
(tests/cpp/test_read_write_core.cpp) and held to the model of the predicate (tests/read_write_model.py): the whole
format walk — wide and plain — over the cases at every alignment of the texts, the records and the output, with every
buffer ending at its last byte; the name span, the segment table, the pieces and the capacity, also above 2^32.
Nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

from genefuserust_amd import read_write   # noqa: F401  (the feature these tests are for)
from tests import read_write_model as model
from tests.read_write_cases import KEPT_SMALL, NAME_LENGTHS, UMI_LENGTHS, build, name_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("read_write_core") / "test_read_write_core")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_read_write_core.cpp")], check=True)
    return exe


def hx(b: bytes) -> str:
    return b.hex() or "-"


def run(program, tmp_path, jobs):
    """The program's answers, a list of token lists; it must end clean under the sanitizers."""
    (tmp_path / "jobs").write_text("".join(j + "\n" for j in jobs))
    done = subprocess.run([program, str(tmp_path / "jobs"), str(tmp_path / "answers")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    out = [line.split() for line in (tmp_path / "answers").read_text().splitlines()]
    assert len(out) == len(jobs)
    return out


def _offsets(records):
    return ",".join(map(str, np.concatenate([[0], np.cumsum([len(b) for b, _ in records])]).astype(np.int64)))


def format_job(source, length, gather, texts, finals, pre, leads, junk):
    """``leads``: per side the alignments of the text, the records, the pre-cut records and the output."""
    n = len(finals[0])
    job = "format %d %d %d %d %d %d" % (source, length, gather, len(texts), n, junk)
    for s, text in enumerate(texts):
        a_text, a_rec, a_pre, a_out = leads[s]
        tagged = source != model.NAME
        job += " %d %s %d %s %s %s %d %s %s %d" % (
            a_text, hx(text), a_rec, hx(b"".join(b for b, _ in finals[s])), hx(b"".join(q for _, q in finals[s])),
            _offsets(finals[s]), a_pre, hx(b"".join(b for b, _ in pre[s])) if tagged else "-",
            _offsets(pre[s]) if tagged else "-", a_out)
    return job


def format_want(source, length, texts, finals, pre):
    want = model.format_reads(texts, finals, source, length, pre)
    out = []
    for s in range(len(texts)):
        out += [hx(want.texts[s]), ",".join(map(str, want.offsets[s]))]
    return out + [",".join(map(str, want.totals)), "1"], want


HEADER = open(os.path.join(ROOT, "include", "gf_read_write.h")).read()


def test_known_answer(program, tmp_path):
    """The header's known answer is the model's, and the program's, wide and plain."""
    text = b"@r1 x\nACGT\n+\nFFFF\n"
    finals, pre = [[(b"GT", b"FF")]], [[(b"ACGT", b"FFFF")]]
    want, got_model = format_want(model.READ1, 2, [text], finals, pre)
    assert got_model.texts[0] == b"@r1:AC x\nGT\n+\nFF\n" and '"@r1:AC x\\nGT\\n+\\nFF\\n"' in HEADER
    assert got_model.totals == [1, 2, 17, 0, 0]
    jobs = [format_job(model.READ1, 2, g, [text], finals, pre, [(3, 7, 1, a)], 0x21) for g in (0, 1) for a in (0, 9, 15)]
    for g in run(program, tmp_path, jobs):
        assert g == want
    assert model.capacity(len(text), 1) == len(text) + 1 + 66 and "1 + 32 + 1 + 32" in HEADER


@pytest.mark.parametrize("sides", [1, 2])
def test_format_at_every_alignment(program, tmp_path, sides):
    """Records of every kept length under names of every length, the mates out of step, no tag: all 16 alignments of
    the output, the other buffers at alignments that change with it; a text with and without its final newline; wide and
    plain give the model's bytes, and no byte outside them is touched."""
    rng = np.random.default_rng(41 + sides)
    jobs, wants = [], []
    for a in range(16):
        texts, finals, pre = build(rng, 23, sides, final_newline=a % 2 == 0, kept=KEPT_SMALL)
        leads = [((3 * a + 1 + s) % 16, (5 * a + 2 * s) % 16, 0, (a + 7 * s) % 16) for s in range(sides)]
        want, got_model = format_want(model.NAME, 0, texts, finals, pre)
        assert got_model.totals[0] > 0 and got_model.totals[4] > 0
        if sides == 2:   # only R1 empty, only R2 empty
            lens = [(len(l[0]), len(r[0])) for l, r in zip(*finals)]
            assert any(x == 0 and y > 0 for x, y in lens) and any(x > 0 and y == 0 for x, y in lens)
        for gather in (model.WIDE, model.BYTES):
            jobs.append(format_job(model.NAME, 0, gather, texts, finals, pre, leads, (0x00, 0xFF, 0x0A, 0x40)[a % 4]))
            wants.append(want)
    for g, w, j in zip(run(program, tmp_path, jobs), wants, jobs):
        assert g == w, j[:80]


def test_format_with_tags(program, tmp_path):
    """Every inline source at the UMI lengths 1, 8 and 32, pairs and reads; both mates carry the same tag."""
    rng = np.random.default_rng(43)
    jobs, wants = [], []
    k = 0
    for length in UMI_LENGTHS:
        for source, sides in ((model.READ1, 2), (model.READ2, 2), (model.PER_READ, 2), (model.READ1, 1),
                              (model.PER_READ, 1)):
            k += 1
            texts, finals, pre = build(rng, 16, sides, source, length, skip=k % 3, final_newline=k % 2 == 0,
                                       kept=KEPT_SMALL)
            want, got_model = format_want(source, length, texts, finals, pre)
            assert got_model.totals[0] > 0 and got_model.totals[4] > 0
            leads = [((k + s) % 16, (3 * k + s) % 16, (7 * k + 5 * s) % 16, (11 * k + 3 * s) % 16) for s in range(sides)]
            jobs.append(format_job(source, length, k % 2, texts, finals, pre, leads, 0x3A))
            wants.append(want)
            if sides == 2:
                i = got_model.written.index(True)
                first = [got_model.texts[s][:got_model.offsets[s][i + 1]].split(b"\n")[-5] for s in (0, 1)]
                t = model.tag(source, length, [pre[0][i][0], pre[1][i][0]])
                assert len(t) == (2 + 2 * length if source == model.PER_READ else 1 + length)
                assert all(t in line for line in first)
    for g, w, j in zip(run(program, tmp_path, jobs), wants, jobs):
        assert g == w, j[:80]


def test_all_dropped_and_empty(program, tmp_path):
    q = b"F" * 8
    text = b"@a\nACGTACGT\n+\nFFFFFFFF\n@b\nAC\n+\nFF\n"
    none = [[(b"", b""), (b"", b"")]]
    jobs = [format_job(model.NAME, 0, 0, [text], none, none, [(1, 2, 3, 4)], 0x55),
            format_job(model.NAME, 0, 0, [b""], [[]], [[]], [(0, 0, 0, 5)], 0x55),
            format_job(model.NAME, 0, 1, [text, text], [[(b"ACGTACGT", q), (b"", b"")], [(b"", b""), (b"AC", q[:2])]],
                       none * 2, [(0, 0, 0, 0), (9, 9, 9, 9)], 0x55)]
    got = run(program, tmp_path, jobs)
    assert got[0] == ["-", "0,0,0", "0,0,0,0,2", "1"]
    assert got[1] == ["-", "0", "0,0,0,0,0", "1"]
    assert got[2] == ["-", "0,0,0", "-", "0,0,0", "0,0,0,0,2", "1"]


def test_token_end_and_name_span(program, tmp_path):
    rng = np.random.default_rng(47)
    lines = [name_line(rng, length, kind) for length in NAME_LENGTHS for kind in range(4)] + [b"", b" ", b"\t@", b"@x"]
    got = run(program, tmp_path, ["token %d %s" % (k % 16, hx(line)) for k, line in enumerate(lines)])
    assert [int(g[0]) for g in got] == [model.token_end(line) for line in lines]
    assert any(model.token_end(line) < len(line) for line in lines) and any(model.token_end(line) == len(line) for line in lines)
    text = b"@a:AC\nAC\n+\nFF\n@b:GT\nGT\n+\nFF\n@c:TT\nTT\n+\nFF"      # no final newline
    nl = [k for k, ch in enumerate(text) if ch == 10]
    got = run(program, tmp_path, ["span %d %d %s" % (len(text), i, " ".join(map(str, nl))) for i in range(5)] +
              ["span 0 0", "span %d 2 %s" % (text.index(b"@c:TT") + 5," ".join(map(str, nl[:8])))])
    for i in range(3):
        s, e = int(got[i][0]), int(got[i][1])
        assert text[s:e] == model.name_line(text, i) != b""
    assert got[0][0] == "0"
    assert got[3] == got[4] == [str(len(text))] * 2 and model.name_line(text, 3) == b""    # no such line: empty, at the end
    assert got[5] == ["0", "0"]
    assert text[int(got[6][0]):int(got[6][1])] == b"@c:TT"     # a text that ends with a name line, no newline behind it


def test_offsets_above_two_to_the_32(program, tmp_path):
    """The span, the segment table, the size and the capacity with offsets above 2^32, fed by hand."""
    G = 1 << 32
    nl = [5 * G + k for k in (10, 20, 30, 40, 50)]
    got = run(program, tmp_path, [
        "span %d 1 %s" % (5 * G + 57, " ".join(map(str, nl))), "span %d 0 %s" % (5 * G + 57, " ".join(map(str, nl))),
        "record %d %d 7 9 %d %d" % (5 * G + 41, 5 * G + 50, 6 * G + 3, 3 * G),
        "size %d 66 %d" % (G + 1, 2 * G), "cap %d %d" % (7 * G, G // 2)])
    assert got[0] == [str(5 * G + 41), str(5 * G + 50)] and got[1] == ["0", str(5 * G + 10)]
    starts = [0, 7, 16, 18, 19, 19 + 3 * G, 22 + 3 * G, 23 + 6 * G]
    assert got[2][0] == ",".join(map(str, starts))
    assert got[3] == [str(G + 1 + 66 + 4 * G + 5)] and got[4] == [str(7 * G + 1 + (G // 2) * 66)]


def test_segment_table_and_pieces(program, tmp_path):
    """The segment of the first and last byte of every segment; the pieces of records of every size at every alignment,
    from the definition: piece q is the 16 addresses from 16 q, the record the ``size`` addresses from ``a``."""
    got = run(program, tmp_path, ["record 100 120 6 9 50 4", "record 100 120 20 0 50 1", "record 0 0 0 0 0 1"])
    assert got[0][0] == "0,6,15,29,30,34,37,42"
    # position 0; then per boundary the byte in front of it and the byte at it
    assert got[0][1] == "0,0,1,1,2,2,3,3,4,4,5,5,6,6"
    assert got[1][0] == "0,20,20,20,21,22,25,27"       # no tag: the head is the whole name, tag and tail are empty
    assert got[2][0] == "0,0,0,0,1,2,5,7" and got[2][1].endswith("5,6,6")
    cases = [(a, size) for a in range(16) for size in (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 355)]
    answers = run(program, tmp_path, ["pieces %d %d" % c for c in cases] + ["pieces 5 0"])
    assert answers[-1] == ["0"]
    for (a, size), g in zip(cases, answers):
        want = []
        for q in range((a + size + 15) // 16):
            inside = [k for k in range(16) if a <= 16 * q + k < a + size]
            assert inside
            full = len(inside) == 16
            want.append("%d:%d:%d:%d" % (16 * q - a, full, inside[0], inside[-1] + 1))
        assert g == [str(len(want))] + want, (a, size)


def test_settings(program, tmp_path):
    settings = [(s, le, g) for s in (-1, 0, 1, 2, 3, 4) for le in (-1, 0, 1, 32, 33) for g in (-1, 0, 1, 2)]
    got = run(program, tmp_path, ["settings %d %d %d" % x for x in settings])
    assert [int(g[0]) for g in got] == [int(model.settings_ok(*x)) for x in settings]
    assert sum(int(g[0]) for g in got) == 2 * (1 + 3 * 2)
