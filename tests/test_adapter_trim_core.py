"""The arithmetic of libgfadapt.so on the host: genefuserust_amd/scan_csrc/gf_at_core.h, the very text the kernels run,
compiled with g++ under AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone program
(tests/cpp/test_adapter_trim_core.cpp) and held to the model of the predicate (tests/adapter_trim_model.py): the walk
of a pair in rounds of 16 and of 64 candidates, at every alignment of the mates' first bytes, with a neighbour's bytes
around them."""
import os
import subprocess

import numpy as np
import pytest

from tests.adapter_trim_cases import (SETTINGS, adapter_reads, modelled, pair_cases, random_pairs, single_cases,
                                      tandem_pair)
from tests.adapter_trim_model import (BY_OVERLAP, BY_SEQUENCE, OVERLAP_CLEAN, TRUSEQ_R1, UNTOUCHED, Settings,
                                      accepted_inserts, adapter_position, decide, overlap_diff)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JUNK = [ord("G"), ord("A"), ord("T"), 0, 255, ord("N")]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("adapter_trim_core") / "test_adapter_trim_core")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_adapter_trim_core.cpp")], check=True)
    return exe


def hx(b: bytes) -> str:
    return b.hex() or "-"


def words(s: Settings, r1_len=None, r2_len=None) -> str:
    return "%d %d %d %d %d %d %d %s %s" % (s.overlap, s.min_overlap, s.max_diff, s.diff_percent, s.min_adapter,
                                           len(s.adapter_r1) if r1_len is None else r1_len,
                                           len(s.adapter_r2) if r2_len is None else r2_len, hx(s.adapter_r1),
                                           hx(s.adapter_r2))


def run(program, tmp_path, jobs):
    """The program's answers, a list of token lists; it must end clean under the sanitizers."""
    (tmp_path / "jobs").write_text("".join(j + "\n" for j in jobs))
    done = subprocess.run([program, str(tmp_path / "jobs"), str(tmp_path / "answers")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    out = [line.split() for line in (tmp_path / "answers").read_text().splitlines()]
    assert len(out) == len(jobs)
    return out


def held_to_the_model(program, tmp_path, records, verdicts, s: Settings, sides: int):
    """Every record at every alignment 0 .. 15 of its first byte (the mate's runs through all 16 too), in rounds of 16
    and of 64."""
    jobs, want = [], []
    for k, ((a, b), verdict) in enumerate(zip(records, verdicts)):
        for al in range(16):
            G, ar, junk = (16, 64)[(al + k) & 1], (5 * al + 3) % 16, JUNK[(al + k) % len(JUNK)]
            jobs.append("pair %d %d %d %d %d %s %s %s" % (G, sides, al, ar, junk, hx(a), hx(b), words(s)))
            want.append(verdict)
    got = run(program, tmp_path, jobs)
    for verdict, g, j in zip(want, got, jobs):
        flat = [x for pair in verdict for x in pair] + ([0, UNTOUCHED] if sides == 1 else [])
        assert [int(x) for x in g] == flat, j[:300]


@pytest.mark.parametrize("name", list(SETTINGS))
def test_pairs_against_the_model(program, tmp_path, name):
    held_to_the_model(program, tmp_path, pair_cases(name), modelled(name), SETTINGS[name], 2)
    seen = {how for verdict in modelled(name) for _, how in verdict}
    assert {BY_OVERLAP, OVERLAP_CLEAN, UNTOUCHED} <= seen or name == "sequence only"
    if name in ("illumina", "sequence only"):
        assert BY_SEQUENCE in seen


@pytest.mark.parametrize("name", ["illumina", "sequence only", "percent 10", "smallest"])
def test_single_end_reads_against_the_model(program, tmp_path, name):
    reads = single_cases(name)
    held_to_the_model(program, tmp_path, [(x, b"") for x in reads], modelled(name, True), SETTINGS[name], 1)
    assert {how for ((_, how),) in modelled(name, True)} == {UNTOUCHED, BY_SEQUENCE}
    assert any(kept == 0 and how == BY_SEQUENCE for ((kept, how),) in modelled(name, True))   # p = 0


def test_the_model_itself():
    """The edges the cases are built around, on the model's answer: so that the comparisons above cover them."""
    s, rng = Settings(), np.random.default_rng(2)
    from tests.adapter_trim_cases import bases_of, read_through, with_diffs
    # the quick loop of accepted_inserts is the definition
    for a, b in random_pairs(6, 4, s, 70):
        for insert in range(s.min_overlap, len(a) + len(b) - s.min_overlap + 1):
            ov, d = overlap_diff(a, b, insert)
            ok = ov >= s.min_overlap and d <= s.max_diff and 100 * d <= s.diff_percent * ov
            assert ok == (insert in accepted_inserts(a, b, s))
    # inserts around min_overlap, the read length and the last candidate
    want = {29: None, 30: 30, 31: 31, 149: 149, 150: 150, 151: 151, 270: 270, 271: None}
    for insert, found in want.items():
        a, b = read_through(rng, bases_of(rng, insert), 150, 150, s)
        got = accepted_inserts(a, b, s)
        assert (max(got) if got else None) == found, insert
    # max_diff, and the percentage biting first: 30 positions at 20 % allow 6, max_diff 5; at 10 % they allow 3
    a, b = read_through(rng, bases_of(rng, 30), 150, 150, s)
    for k, default, ten, wide in ((0, 1, 1, 1), (3, 1, 1, 1), (4, 1, 0, 1), (5, 1, 0, 1), (6, 0, 0, 1), (7, 0, 0, 0)):
        x = with_diffs(a, range(2, 2 + k))
        assert (30 in accepted_inserts(x, b, s)) == bool(default)
        assert (30 in accepted_inserts(x, b, s._replace(diff_percent=10))) == bool(ten)
        assert (30 in accepted_inserts(x, b, s._replace(max_diff=10))) == bool(wide)
    # a tandem repeat of period 7: several accepted inserts, the largest is taken
    a, b = tandem_pair(rng, s)
    got = accepted_inserts(a, b, s)
    assert len(got) > 1 and 98 in got and {y - x for x, y in zip(got, got[1:])} == {7}
    assert decide(a, b, s) == [(max(got), BY_OVERLAP)] * 2 and max(got) >= 98
    # N and lower case
    a, b = read_through(rng, bases_of(rng, 100), 150, 150, s)
    assert decide(a.lower(), b, s)[0] == (100, BY_OVERLAP)
    assert overlap_diff(a[:50] + b"N" + a[51:], b, 100) == (100, 1)
    # the sequence step: floor(n / 10) differences pass, one more does not; a cut-off adapter; p = 0
    t = s._replace(adapter_r1=TRUSEQ_R1)
    x = bases_of(rng, 100) + TRUSEQ_R1 + bases_of(rng, 17)
    assert adapter_position(x, TRUSEQ_R1, t) == 100
    assert adapter_position(with_diffs(x, (101, 110, 120)), TRUSEQ_R1, t) == 100
    assert adapter_position(with_diffs(x, (101, 110, 120, 130)), TRUSEQ_R1, t) is None
    assert adapter_position(x[:110], TRUSEQ_R1, t) == 100 and adapter_position(x[:109], TRUSEQ_R1, t) is None
    assert adapter_position(x[:110].lower(), TRUSEQ_R1, t) == 100
    assert adapter_position(x[:104] + b"N" + x[105:110], TRUSEQ_R1, t) == 100   # one difference in ten
    assert adapter_position(x[:104] + b"NN" + x[106:119], TRUSEQ_R1, t) is None   # two in nineteen
    assert decide(TRUSEQ_R1 + b"ACGT", None, t) == [(0, BY_SEQUENCE)]
    assert decide(b"A" * 150, None, t) == [(150, UNTOUCHED)]
    assert decide(b"A" * 513, b"T" * 100, s) == [(513, UNTOUCHED), (100, UNTOUCHED)]
    assert len(adapter_reads(t)) > 100


def test_settings(program, tmp_path):
    ok = SETTINGS["illumina"]
    a1 = ok.adapter_r1
    bad = [words(ok._replace(overlap=2)), words(ok._replace(overlap=-1)), words(ok._replace(min_overlap=7)),
           words(ok._replace(min_overlap=513)), words(ok._replace(max_diff=-1)), words(ok._replace(diff_percent=101)),
           words(ok._replace(diff_percent=-1)), words(ok._replace(min_adapter=3)), words(ok._replace(min_adapter=65)),
           words(ok, r1_len=9), words(ok, r2_len=65), words(ok, r1_len=-1),
           words(ok._replace(adapter_r1=a1[:5] + b"N" + a1[6:])), words(ok._replace(adapter_r2=a1.lower())),
           words(ok._replace(adapter_r1=a1[:5] + b"\x00" + a1[6:])),
           words(Settings(overlap=0)), words(ok._replace(min_adapter=34))]
    fine = [words(ok), words(Settings()), words(SETTINGS["smallest"]), words(SETTINGS["sequence only"]),
            words(Settings(min_overlap=512, max_diff=2 ** 31 - 1, diff_percent=100, min_adapter=64,
                           adapter_r2=SETTINGS["smallest"].adapter_r2))]
    got = run(program, tmp_path, ["settings 0 " + w for w in bad + fine])
    assert all(g != ["ok"] for g in got[:len(bad)]) and got[len(bad):] == [["ok"]] * len(fine), got
    # single-end input needs adapter_r1
    got = run(program, tmp_path, ["settings 1 " + words(Settings()), "settings 1 " + words(Settings(adapter_r2=a1)),
                                  "settings 1 " + words(ok)])
    assert got[0] != ["ok"] and got[1] != ["ok"] and got[2] == ["ok"]
