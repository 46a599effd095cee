"""The arithmetic of libgfcorrect.so on the host: genefuserust_amd/scan_csrc/gf_oc_core.h, the very text the kernel
runs, compiled with g++ under AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone program
(tests/cpp/test_overlap_correct_core.cpp) and held to the model of the predicate (tests/overlap_correct_model.py): the
walk of a pair in rounds of 16 and of 64 candidates, at every alignment of the mates' first bytes, with a neighbour's
bytes around the records."""
import os
import subprocess

import numpy as np
import pytest

from tests.adapter_trim_cases import spread
from tests.overlap_correct_cases import SETTINGS, Pair, bad_q, cases, good_q, modelled
from tests.overlap_correct_model import FIX_R1, FIX_R2, LEFT, Settings, correct_batch, correct_pair, decide, settings_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JUNK = [ord("G"), ord("A"), ord("T"), 0, 255, ord("N")]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("overlap_correct_core") / "test_overlap_correct_core")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_overlap_correct_core.cpp")], check=True)
    return exe


def hx(b: bytes) -> str:
    return b.hex() or "-"


def words(s: Settings) -> str:
    return "%d %d %d %d %d" % s


def run(program, tmp_path, jobs):
    """The program's answers, a list of token lists; it must end clean under the sanitizers."""
    (tmp_path / "jobs").write_text("".join(j + "\n" for j in jobs))
    done = subprocess.run([program, str(tmp_path / "jobs"), str(tmp_path / "answers")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    out = [line.split() for line in (tmp_path / "answers").read_text().splitlines()]
    assert len(out) == len(jobs)
    return out


@pytest.mark.parametrize("name", list(SETTINGS))
def test_pairs_against_the_model(program, tmp_path, name):
    """Every case at every alignment 0 .. 15 of R1's first byte (R2's runs through all 16 too), in rounds of 16 and of
    64: bases, qualities, I* and the counts are the model's, the difference words sum to the search's count, and the
    neighbours' bytes are as they were."""
    s = SETTINGS[name]
    jobs, want = [], []
    for k, (case, answer) in enumerate(zip(cases(name), modelled(name))):
        for al in range(16):
            G, ar, junk = (16, 64)[(al + k) & 1], (5 * al + 3) % 16, JUNK[(al + k) % len(JUNK)]
            jobs.append("pair %d %d %d %d %s %s %s %s %s" % (G, al, ar, junk, *[hx(x) for x in case], words(s)))
            want.append(answer)
    got = run(program, tmp_path, jobs)
    for c, g, j in zip(want, got, jobs):
        assert [int(x) for x in g[:5]] == [c.insert, c.fixed[0], c.fixed[1], c.left, 1], j[:200]
        assert g[5:9] == [hx(c.a), hx(c.qa), hx(c.b), hx(c.qb)], j[:200]
        assert g[9] == "1", j[:200]


def test_the_model_itself():
    """Every branch and every total is reached, on the model's answer: so that the comparisons above and on the device
    cover them."""
    for name, s in SETTINGS.items():
        answers = modelled(name)
        seen = {b for c in answers for b in c.branches}
        assert seen == {"r1", "r2", "left"}, name
        totals = correct_batch([c[:2] for c in cases(name)], [c[2:] for c in cases(name)], s, answers).totals
        assert totals[0] == len(cases(name)) and all(t > 0 for t in totals), (name, totals)
        assert totals[1] < totals[0] and totals[2] < totals[1]          # pairs without an I*, and without a difference
        assert any(c.fixed[0] and c.fixed[1] for c in answers)          # both mates in one pair
        assert any(sum(c.fixed) and c.left for c in answers)            # corrected beside a difference left standing
    s, rng = Settings(), np.random.default_rng(3)
    good, bad = 33 + s.good_phred, 33 + s.bad_phred
    # the thresholds, on either side
    assert decide(ord("A"), good, ord("A"), bad, s) == FIX_R2 and decide(ord("A"), bad, ord("A"), good, s) == FIX_R1
    assert decide(ord("A"), good - 1, ord("A"), bad, s) == LEFT and decide(ord("A"), good, ord("A"), bad + 1, s) == LEFT
    assert decide(ord("A"), bad, ord("A"), good - 1, s) == LEFT and decide(ord("A"), bad + 1, ord("A"), good, s) == LEFT
    assert decide(ord("A"), good, ord("A"), good, s) == LEFT and decide(ord("A"), bad, ord("A"), bad, s) == LEFT
    # a quality byte below 33 is phred 0
    assert decide(ord("A"), good, ord("C"), 0, s) == FIX_R2 and decide(ord("A"), 32, ord("C"), 32, s) == LEFT
    # N: corrected when low, never a source
    assert decide(ord("N"), bad, ord("C"), good, s) == FIX_R1 and decide(ord("C"), good, ord("n"), bad, s) == FIX_R2
    assert decide(ord("N"), good, ord("C"), bad, s) == LEFT and decide(ord("C"), bad, ord("N"), good, s) == LEFT
    # what is written: the upper-case complement and the source's quality; lengths stay
    c = correct_pair(*Pair(rng, s, 100).miscall(40, 1).case(), s)
    p = Pair(rng, s, 100)
    p.a = bytearray(bytes(p.a).lower())
    src = p.a[40]
    c = correct_pair(*p.miscall(40, 1, 40, 70).case(), s)
    assert c.branches == ("r2",) and c.b[59] == ord({"a": "T", "c": "G", "g": "C", "t": "A"}[chr(src)]) and c.qb[59] == 70
    assert c.insert == 100 and c.fixed == (0, 1) and (len(c.a), len(c.b)) == (150, 150)
    # the positions: lo, hi - 1 and the word boundaries, with I* above the read length too
    for I in (100, 166):
        lo, hi = max(0, I - 150), min(I, 150)
        for i in sorted({lo, hi - 1, 31, 32, 63, 64} & set(range(lo, hi))):
            for side in (0, 1):
                c = correct_pair(*Pair(rng, s, I).miscall(i, side).case(), s)
                assert c.insert == I and c.fixed == ((1, 0), (0, 1))[side] and c.left == 0, (I, i, side)
    # d = max_diff: all corrected; one more: no I*, untouched
    for k in (s.max_diff, s.max_diff + 1):
        p = Pair(rng, s, 100)
        for i in spread(rng, 0, 100, k):
            p.miscall(i, i & 1)
        c = correct_pair(*p.case(), s)
        assert (c.insert, sum(c.fixed)) == ((100, k) if k == s.max_diff else (-1, 0))
        assert k == s.max_diff or (c.a, c.qa, c.b, c.qb) == p.case()
    # the limits
    assert correct_pair(b"A" * 513, b"I" * 513, b"T" * 100, b"#" * 100, s).insert == -1
    assert correct_pair(b"", b"", b"T" * 100, b"#" * 100, s).insert == -1
    assert good_q(s) - 33 >= s.good_phred and bad_q(s) - 33 <= s.bad_phred


def test_settings(program, tmp_path):
    ok = Settings()
    bad = [ok._replace(min_overlap=7), ok._replace(min_overlap=513), ok._replace(max_diff=-1),
           ok._replace(diff_percent=-1), ok._replace(diff_percent=101), ok._replace(good_phred=94),
           ok._replace(good_phred=-1), ok._replace(bad_phred=-1), ok._replace(bad_phred=94, good_phred=93),
           ok._replace(bad_phred=30), ok._replace(bad_phred=31), ok._replace(good_phred=0, bad_phred=0)]
    fine = [ok, *SETTINGS.values(), Settings(8, 0, 0, 1, 0), Settings(512, 2 ** 31 - 1, 100, 93, 92)]
    assert all(settings_error(s) for s in bad) and not any(settings_error(s) for s in fine)
    got = run(program, tmp_path, ["settings " + words(s) for s in bad + fine])
    assert all(g != ["ok"] for g in got[:len(bad)]) and got[len(bad):] == [["ok"]] * len(fine), got
