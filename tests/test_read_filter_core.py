"""The arithmetic of libgfprep.so on the host: genefuserust_amd/scan_csrc/gf_pp_core.h, the very text the kernels run,
compiled with g++ under AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone program
(tests/cpp/test_read_filter_core.cpp) and held to the model of the predicate (tests/read_filter_model.py): the walk of
a read in tiles of 16 and of 64 chunks, at every alignment of its first byte, with a neighbour's bytes around it."""
import os
import subprocess

import numpy as np
import pytest

from tests.read_filter_cases import SETTINGS, edge_reads, random_reads
from tests.read_filter_model import Settings, decide

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JUNK = [ord("G"), ord("A"), 0, 255, 33 + 40]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("read_filter_core") / "test_read_filter_core")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_read_filter_core.cpp")], check=True)
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


def job(rng, b: bytes, q: bytes, s: Settings, G: int) -> str:
    ab, aq = (int(x) for x in rng.integers(0, 16, 2))
    jb, jq = (JUNK[int(x)] for x in rng.integers(0, len(JUNK), 2))
    return "read %d %d %d %d %d %s %s %s" % (G, ab, aq, jb, jq, hx(b), hx(q), " ".join(str(x) for x in s))


def held_to_the_model(program, tmp_path, reads, s: Settings, seed: int):
    rng = np.random.default_rng(seed)
    jobs, want = [], []
    for b, q in reads:
        for G in ((16, 64) if len(b) <= 600 else (16 if rng.integers(0, 2) else 64,)):
            jobs.append(job(rng, b, q, s, G))
            want.append(decide(b, q, s))
    got = run(program, tmp_path, jobs)
    for (e2, reason), g, j in zip(want, got, jobs):
        assert [int(x) for x in g] == [e2, reason], j[:200]
    return want


@pytest.mark.parametrize("name", list(SETTINGS))
def test_edge_reads_against_the_model(program, tmp_path, name):
    s = SETTINGS[name]
    want = held_to_the_model(program, tmp_path, edge_reads(s), s, 3)
    if name in ("defaults", "window 4"):   # every reason occurs, and both trims
        assert {r for _, r in want} == {0, 1, 2, 3}


def test_random_reads_against_the_model(program, tmp_path):
    reads = random_reads(1500, 11) + random_reads(40, 12, longest=4200)
    seen = set()
    for k, name in enumerate(("defaults", "window 4", "window 64", "no poly-G")):
        part = reads[k::4]
        want = held_to_the_model(program, tmp_path, part, SETTINGS[name], 20 + k)
        seen |= {r for _, r in want}
        assert sum(e2 < len(b) for (e2, r), (b, _) in zip(want, part) if r == 0) > 10   # kept and shortened
    assert seen == {0, 1, 2, 3}


def test_every_alignment_of_one_read(program, tmp_path):
    """A read whose window lies where two tiles of the window step overlap, at all 16 x 16 alignments."""
    s = Settings(cut_tail_window=64, cut_tail_mean=30, poly_g_min=10)
    b = b"ACGT" * 100 + b"G" * 12
    for at in (0, 70, 150, 176, 200, 330):
        q = bytes([35]) * at + bytes([33 + 30]) * 64 + bytes([35]) * (len(b) - at - 64)
        jobs = ["read %d %d %d 71 126 %s %s %s" % (G, ab, aq, hx(b), hx(q), " ".join(str(x) for x in s))
                for G in (16, 64) for ab in range(16) for aq in range(16)]
        assert {tuple(g) for g in run(program, tmp_path, jobs)} == {tuple(str(x) for x in decide(b, q, s))}
        assert decide(b, q, s)[0] == at + 64


def test_pair_rule_and_settings(program, tmp_path):
    got = run(program, tmp_path, ["pair %d %d" % (l, r) for l in range(4) for r in range(4)])
    for (l, r), g in zip([(l, r) for l in range(4) for r in range(4)], got):
        want = (l or (4 if r else 0), r or (4 if l else 0))
        assert tuple(int(x) for x in g) == want
    ok = Settings()
    bad = [ok._replace(**{f: -1}) for f in ok._fields]
    bad += [ok._replace(cut_tail_window=65), ok._replace(cut_tail_mean=94), ok._replace(qualified_phred=94),
            ok._replace(unqualified_percent=101), ok._replace(poly_g_min=4097), ok._replace(length_required=4097)]
    fine = [ok, SETTINGS["largest"], Settings(0, 0, 0, 0, 0, 0, 0)]
    got = run(program, tmp_path, ["settings " + " ".join(str(x) for x in s) for s in bad + fine])
    assert all(g != ["ok"] for g in got[:len(bad)]) and got[len(bad):] == [["ok"]] * len(fine)
