"""The arithmetic of libgfqc.so on the host: genefuserust_amd/scan_csrc/gf_qc_core.h, the very text the kernels run,
compiled with g++ under AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone program
(tests/cpp/test_read_qc_core.cpp) and held to the model of the tables (tests/read_qc_model.py): the walk of a record
lane after lane, at every alignment of its first byte, with a neighbour's bytes around it; and a pair's entry of the
insert histogram over gf_at_core.h.  Nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

from genefuserust_amd import read_qc   # noqa: F401  (the feature these tests are for)
from tests.read_qc_cases import LENGTHS, edge_reads, insert_entries, insert_pairs, short_reads
from tests.read_qc_model import SIDE_WORDS, stats_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JUNK = [ord("G"), ord("A"), 0, 255, 33 + 40]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("read_qc_core") / "test_read_qc_core")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_read_qc_core.cpp")], check=True)
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


def table_of(tokens) -> np.ndarray:
    t = np.zeros(SIDE_WORDS, dtype=np.int64)
    for tok in tokens:
        w, v = tok.split("=")
        t[int(w)] = int(v)
    return t


def test_every_alignment_of_every_edge_length(program, tmp_path):
    """One read of each length of the cases up to 600, at all 16 alignments, junk around it."""
    reads = [r for r in edge_reads() if len(r[0]) <= 600][:len([n for n in LENGTHS if n <= 600]) * 2]
    jobs, want = [], []
    for k, (b, q) in enumerate(reads):
        for a in range(16):
            jobs.append("read %d %d %d %s %s" % (a, JUNK[(k + a) % 5], JUNK[(k + 2 * a) % 5], hx(b), hx(q)))
            want.append(stats_table([(b, q)]))
    assert {len(b) for b, _ in reads} == {n for n in LENGTHS if n <= 600}
    for g, w, j in zip(run(program, tmp_path, jobs), want, jobs):
        assert np.array_equal(table_of(g), w), j[:120]


def test_long_and_short_reads_against_the_model(program, tmp_path):
    """The tail row over many rounds, and short reads; every column of the table occurs."""
    rng = np.random.default_rng(4)
    reads = [r for r in edge_reads() if len(r[0]) > 600] + list(short_reads(300))
    jobs = ["read %d %d %d %s %s" % (int(rng.integers(0, 16)), JUNK[k % 5], JUNK[(k + 1) % 5], hx(b), hx(q))
            for k, (b, q) in enumerate(reads)]
    total = np.zeros(SIDE_WORDS, dtype=np.int64)
    for g, (b, q), j in zip(run(program, tmp_path, jobs), reads, jobs):
        assert np.array_equal(table_of(g), stats_table([(b, q)])), j[:120]
        total += table_of(g)
    assert np.array_equal(total, stats_table(reads))
    cycles = total[513:].reshape(513, 8)
    assert (cycles[0] > 0).all() and (cycles[512] > 0).all() and total[512] == 4 and total[1:41].sum() == 300


def test_offsets_and_rows(program, tmp_path):
    cases = [(0, 0), (5, 5), (7, 3), (100, 0), (3, 4), (10, 521), (10, 522), (10, 523), (0, 1 << 40)]
    for (start, end), g in zip(cases, run(program, tmp_path, ["offsets %d %d" % c for c in cases])):
        L = max(end - start, 0)
        assert [int(x) for x in g] == [L, min(L, 512)]
    positions = [0, 1, 63, 64, 511, 512, 513, 1 << 33]
    for pos, g in zip(positions, run(program, tmp_path, ["row %d" % p for p in positions])):
        assert [int(x) for x in g] == [min(pos, 512), 513 + 8 * min(pos, 512)]


def test_insert_entries_against_the_model(program, tmp_path):
    pairs, want = insert_pairs(), insert_entries()
    rng = np.random.default_rng(6)
    jobs = ["pair %d %d %d %s %s" % (int(rng.integers(0, 16)), int(rng.integers(0, 16)), JUNK[k % 5], hx(a), hx(b))
            for k, (a, b) in enumerate(pairs)]
    got = [int(g[0]) for g in run(program, tmp_path, jobs)]
    assert got == list(want)
    assert want[-3:] == (994, 900, 30) and 1025 in want and 0 in want
    assert all(x == 0 or 30 <= x <= 994 or x == 1025 for x in got)
