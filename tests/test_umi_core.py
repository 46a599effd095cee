"""The arithmetic of libgfumi.so on the host: genefuserust_amd/scan_csrc/gf_um_core.h, the very text the kernels run,
compiled with g++ under AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone program
(tests/cpp/test_umi_core.cpp) and held to the model of the predicate (tests/umi_model.py): the cut of a record at every
(length, skip) of the grid, at the lengths around the UMI's and at every alignment of its first byte, the name parser on
every name case with the buffer ending at the line's last byte, and the key mixing.  Nothing loaded into Python runs
under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

from genefuserust_amd import umi   # noqa: F401  (the feature these tests are for)
from tests import umi_model as model
from tests.umi_cases import GRID, JUNK, NAME_CASES, record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("umi_core") / "test_umi_core")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_umi_core.cpp")], check=True)
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


def cut_job(source, length, skip, rec, a1, a2, junk):
    pair = isinstance(rec[0], tuple)
    r1, r2 = (rec[0][0], rec[1][0]) if pair else (rec[0], b"")
    return "cut %d %d %d %d %d %d %d %s %s" % (source, length, skip, 2 if pair else 1, a1, a2, junk, hx(r1), hx(r2))


def cut_want(source, length, skip, rec):
    """What the program answers for one record, from the model."""
    pair = isinstance(rec[0], tuple)
    got = model.cut(source, length, skip, [rec])
    new = got.records[0] if pair else (got.records[0],)
    old = rec if pair else (rec,)
    stays = got.totals[5] == 0
    cuts = [len(o[0]) - len(n[0]) for o, n in zip(old, new)] + ([] if pair else [0])
    return [str(int(stays)), str(cuts[0]), str(cuts[1]), "%016x" % got.codes[0], str(got.totals[3])]


HEADER = open(os.path.join(ROOT, "include", "gf_umi.h")).read()


def test_known_answers(program, tmp_path):
    """The header's known answers are the model's, and the program's."""
    a, p, f = model.code(b"ACGTACGT"), model.code_pair(b"ACGT", b"TTGA"), model.code(b"ACGT+TTGA")
    K = model.key(b"ACGT")
    assert a == model.code(b"acgtacgt") == 0x1d189c7f508326f9 and p == 0x8a0ec19742ea7304 and f == 0xdecfd2a34e770449
    assert K == 0xab0fcab10dd0c6f9
    mixed = [model.mix_key(K, u) for u in (a, p, f)]
    assert mixed == [0xff1a16f0056acf7f, 0xf6e69183b4f4f21c, 0xc7033d0180ee6594]
    for x in [a, p, f, K] + mixed:
        assert "0x%016x" % x in HEADER
    q = b"I" * 12
    got = run(program, tmp_path, [
        cut_job(model.READ1, 8, 0, (b"ACGTACGT", q[:8]), 0, 0, 0), cut_job(model.READ1, 8, 0, (b"acgtacgt", q[:8]), 7, 0, 255),
        cut_job(model.PER_READ, 4, 0, ((b"ACGT", q[:4]), (b"TTGA", q[:4])), 3, 9, 71),
        "name 5 58 %s" % hx(b"@r:ACGT+TTGA"), "mix %x %x" % (K, a), "mix %x %x" % (K, p), "mix %x %x" % (K, f),
        "mix 0 %x" % a, "mix %x 0" % K])
    assert got[0] == got[1] == ["1", "8", "0", "%016x" % a, "0"]
    assert got[2] == ["1", "4", "4", "%016x" % p, "0"]
    assert got[3] == ["%016x" % f, "0"]
    assert [g[0] for g in got[4:7]] == ["%016x" % m for m in mixed]
    assert got[7] == ["%016x" % 0] and got[8] == ["%016x" % K]     # K == 0 and U == 0 pass through


def test_cut_on_the_grid_at_every_alignment(program, tmp_path):
    """Every (length, skip) of the grid, the record lengths c - 1, c, c + 1 on a taking side, all 16 alignments of the
    first byte, each source, reads and pairs; the buffers end with the records' last bytes."""
    rng = np.random.default_rng(11)
    jobs, want = [], []
    for length, skip in GRID:
        c = length + skip
        for k, L in enumerate((c - 1, c, c + 1)):
            for a in range(16):
                junk = JUNK[(a + k) % len(JUNK)]
                r1, r2 = record(rng, L), record(rng, c + 3 + a)
                cases = [(model.READ1, r1), (model.PER_READ, r1), (model.READ1, (r1, r2)), (model.READ2, (r2, r1)),
                         (model.PER_READ, (r1, r2)), (model.PER_READ, (r2, r1))]
                source, rec = cases[(a + k) % len(cases)]
                jobs.append(cut_job(source, length, skip, rec, a, (5 * a + 3) % 16, junk))
                want.append(cut_want(source, length, skip, rec))
    got = run(program, tmp_path, jobs)
    assert any(w[0] == "0" for w in want) and any(w[0] == "1" and w[4] == "1" for w in want)
    for g, w, j in zip(got, want, jobs):
        assert g == w, j[:100]


def test_cut_edges(program, tmp_path):
    """Empty records, a mate emptied by the other side's short record, a side that takes nothing and is shorter than
    the UMI, an N in the UMI but not in the spacer."""
    q = b"F" * 40
    cases = [(model.READ1, 8, 2, (b"", b"")), (model.PER_READ, 8, 2, ((b"ACGTACGTAC", q[:10]), (b"ACGTACGTA", q[:9]))),
             (model.READ1, 8, 2, ((b"ACGTACGTACGG", q[:12]), (b"AC", q[:2]))),
             (model.READ2, 8, 2, ((b"AC", q[:2]), (b"ACGTACGTACGG", q[:12]))),
             (model.READ2, 8, 2, ((b"ACGTACGTACGG", q[:12]), (b"AC", q[:2]))),
             (model.READ1, 8, 2, (b"ACGTACNAGG", q[:10])), (model.READ1, 8, 2, (b"ACGTACGnAA", q[:10])),
             (model.READ1, 8, 2, (b"ACGTACGTNNGG", q[:12]))]
    jobs = [cut_job(s, le, sk, rec, 13, 2, 0x4E) for s, le, sk, rec in cases]
    want = [cut_want(s, le, sk, rec) for s, le, sk, rec in cases]
    assert [w[0] for w in want] == ["0", "0", "1", "1", "0", "1", "1", "1"]
    assert [w[4] for w in want[5:]] == ["1", "1", "0"] and want[2][1:3] == ["10", "0"] and want[4][1:3] == ["12", "2"]
    assert run(program, tmp_path, jobs) == want


def test_name_parser_on_every_case(program, tmp_path):
    """Every name case at all 16 alignments, the buffer ending at the line's last byte, junk — a colon and a space among
    it — in front."""
    assert {ord(":"), ord(" ")} <= set(JUNK)
    jobs, want = [], []
    for k, (line, has) in enumerate(NAME_CASES):
        field = model.name_field(line)
        assert (field is not None) == has, line[:60]
        for a in range(16):
            jobs.append("name %d %d %s" % (a, JUNK[(k + a) % len(JUNK)], hx(line)))
            want.append(["%016x" % (model.code(field) if has else 0), str(int(has and model.has_n(field)))])
    for g, w, j in zip(run(program, tmp_path, jobs), want, jobs):
        assert g == w, j[:100]
    upper, lower = (model.name_field(NAME_CASES[k][0]) for k in (1, 3))
    assert upper != lower and model.code(upper) == model.code(lower)


def test_settings_and_name_lines(program, tmp_path):
    settings = [(s, le, sk) for s in (-1, 0, 1, 2, 3, 4) for le in (-1, 0, 1, 32, 33) for sk in (-1, 0, 32, 33)]
    got = run(program, tmp_path, ["settings %d %d %d" % x for x in settings])
    assert [int(g[0]) for g in got] == [int(model.settings_ok(*x)) for x in settings]
    assert sum(int(g[0]) for g in got) == 1 + 3 * 2 * 2
    text = b"@a:AC\nAC\n+\nFF\n@b:GT\nGT\n+\nFF\n@c:TT\nTT\n+\nFF"      # no final newline
    nl = [k for k, ch in enumerate(text) if ch == 10]
    jobs = ["line %d %d %s" % (len(text), i, " ".join(map(str, nl))) for i in range(5)]
    jobs.append("line 0 0")
    got = run(program, tmp_path, jobs)
    for i in range(3):
        s, e = int(got[i][1]), int(got[i][2])
        assert got[i][0] == "1" and text[s:e] == model.name_line(text, i)
    assert got[3][0] == got[4][0] == "0" and model.name_line(text, 3) is None
    assert got[5] == ["1", "0", "0"] and model.name_line(b"", 0) == b""
