"""The arithmetic of libgfdedup.so on the host: genefuserust_amd/scan_csrc/gf_dd_core.h, the very text the kernels run,
compiled with g++ under AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone program
(tests/cpp/test_dedup_core.cpp) and held to the model of the predicate (tests/dedup_model.py): the walk of a record
piece after piece, at every alignment of its first byte, with junk around it; and a single-thread walk of insert, rehash
and histogram over crafted keys.  Nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

from genefuserust_amd import dedup   # noqa: F401  (the feature these tests are for)
from tests import dedup_model as model
from tests.dedup_cases import JUNK, LENGTHS, edge_reads, near_duplicates, random_read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dedup_core") / "test_dedup_core")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_dedup_core.cpp")], check=True)
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


def test_known_answers(program, tmp_path):
    assert model.key(b"ACGT") == model.key(b"acgt") == 0xab0fcab10dd0c6f9
    assert model.key(b"ACGT", b"") == 0xade372bd9e169438 and model.H(b"") == 0
    got = run(program, tmp_path, ["hash 0 0 %s" % hx(b"ACGT"), "hash 5 255 %s" % hx(b"acgt"),
                                  "pair 3 9 71 %s -" % hx(b"ACGT"), "hash 7 71 -", "pair 1 2 0 - -"])
    assert got[0] == got[1] == ["ab0fcab10dd0c6f9"] * 2
    assert got[2] == ["ade372bd9e169438"]
    assert got[3] == ["%016x" % 0] * 2 and got[4] == ["%016x" % 0]   # no bases: H is 0, and there is no key


def test_every_length_at_every_alignment(program, tmp_path):
    """Every length of the cases at all 16 alignments, junk — a NUL, 0xFF and G among it — around the record: the
    buffer ends with the chunk of the record's last byte, so a load past it fails under ASan."""
    reads = edge_reads()[::2]
    assert [len(r) for r in reads] == LENGTHS and {0, 0xFF, ord("G")} <= set(JUNK)
    jobs = ["hash %d %d %s" % (a, JUNK[(k + a) % len(JUNK)], hx(r)) for k, r in enumerate(reads) for a in range(16)]
    want = [["%016x" % model.H(r), "%016x" % model.key(r)] for r in reads for _ in range(16)]
    for g, w, j in zip(run(program, tmp_path, jobs), want, jobs):
        assert g == w, j[:80]


def test_pairs_near_duplicates_and_swapped_mates(program, tmp_path):
    rng = np.random.default_rng(2)
    jobs, want = [], []
    for k, (a, b, same) in enumerate(near_duplicates()):
        assert (model.key(a) == model.key(b)) == same, (a[:20], b[:20])
        for r in (a, b):
            jobs.append("hash %d %d %s" % (int(rng.integers(0, 16)), JUNK[k % len(JUNK)], hx(r)))
            want.append(["%016x" % model.H(r), "%016x" % model.key(r)])
    reads = [r for r in edge_reads() if len(r) <= 300]
    pairs = [(reads[k], reads[-1 - k]) for k in range(len(reads))] + [(b"", reads[5]), (reads[5], b""), (b"", b"")]
    for a, b in pairs:
        if a != b:
            assert model.key(a, b) != model.key(b, a)   # the mates swapped: another key
        jobs.append("pair %d %d %d %s %s" % (int(rng.integers(0, 16)), int(rng.integers(0, 16)), 0xFF, hx(a), hx(b)))
        want.append(["%016x" % model.key(a, b)])
    for g, w, j in zip(run(program, tmp_path, jobs), want, jobs):
        assert g == w, j[:80]


def test_distinct_sequences_have_distinct_keys():
    """A condition on the inputs, not on the code: a 64-bit key joins two of 10^5 distinct reads with probability
    3e-10."""
    rng = np.random.default_rng(5)
    reads = {random_read(rng, int(n)).upper() for n in rng.integers(0, 200, 100_000)} - {b""}
    assert len(reads) > 90_000 and len({model.key(r) for r in reads}) == len(reads)


def test_small_formulas(program, tmp_path):
    masks = [(L, j) for L in (0, 1, 7, 8, 9, 15, 16, 17, 4096, 5000) for j in (0, 1, 2, 511, 512, 624, 625)]
    for (L, j), g in zip(masks, run(program, tmp_path, ["mask %d %d" % m for m in masks])):
        left = min(max(L - 8 * j, 0), 8)
        assert int(g[0], 16) == (1 << 8 * left) - 1, (L, j)
    spans = [(0, 0), (5, 5), (7, 3), (100, 0), (3, 4), (0, 1 << 40)]
    for (s, e), g in zip(spans, run(program, tmp_path, ["length %d %d" % x for x in spans])):
        assert int(g[0]) == max(e - s, 0)
    M = (1 << 64) - 1
    keys = [(1, 1024), (1023, 1024), (0xab0fcab10dd0c6f9, 1024), (0xab0fcab10dd0c6f9, 1 << 31), (M, 4096)]
    for (k, slots), g in zip(keys, run(program, tmp_path, ["home %x %d" % x for x in keys])):
        assert [int(x) for x in g] == [model.home(k, slots), (model.home(k, slots) + 1) % slots]
    assert model.home(M, 4096) == 4095
    counts = [0, 1, 2, 30, 31, 32, 100, (1 << 32) - 1]
    for c, g in zip(counts, run(program, tmp_path, ["level %d" % c for c in counts])):
        assert int(g[0]) == model.level(c)
    sizes = [0, 1, 512, 1023, 1024, 1025, 1536, 2048, 1 << 31, -1024]
    got = [int(g[0]) for g in run(program, tmp_path, ["slots %d" % n for n in sizes])]
    assert got == [0, 0, 0, 0, 1, 0, 0, 1, 1, 0]


def _walk(program, tmp_path, slots, grown, offered, counted=True):
    """The program's table walk over ``offered`` ((key, index) in order): (failed probes, entries, histogram)."""
    job = "table %d %d %d %s" % (slots, grown, int(counted), " ".join("%x:%d" % x for x in offered))
    tokens = run(program, tmp_path, [job])[0]
    bar = tokens.index("|")
    entries = set()
    for tok in tokens[1:bar]:
        k, f, c = tok.split(":")
        entries.add((int(k, 16), int(f), int(c)))
    return int(tokens[0].split("=")[1]), entries, [0] + [int(x) for x in tokens[bar + 1:]]


def test_table_walk_over_crafted_keys(program, tmp_path):
    """One chain that wraps in a half-full table, repeats at lower and higher indices, a rehash, the histogram."""
    slots = 1024
    chain = [(k << 10) | 1023 for k in range(1, 513)]          # 512 keys, all with home slot 1023
    assert {model.home(k, slots) for k in chain} == {1023}
    offered = [(k, 100 + i) for i, k in enumerate(chain)]
    offered += [(chain[0], 5)] * 30 + [(chain[1], 9000)] * 99 + [(chain[2], 7)]
    t = model.Table()
    for k, i in offered:
        t.insert([k], i)
    for grown in (0, 4096):
        failed, entries, hist = _walk(program, tmp_path, slots, grown, offered)
        assert failed == 0 and entries == t.entries() and hist == t.histogram()
    assert t.histogram()[31] == 2 and t.histogram()[2] == 1 and t.histogram()[1] == 509
    assert (chain[0], 5, 31) in t.entries() and (chain[1], 101, 100) in t.entries()
    # nothing counted: the same keys and indices, every count 0, an empty histogram
    failed, entries, hist = _walk(program, tmp_path, slots, 0, offered, counted=False)
    assert failed == 0 and entries == {(k, f, 0) for k, f, _ in t.entries()} and not any(hist)
    # a full table: the next key visits every slot once and gives up
    full = [(k, k) for k in range(1, 1026)]
    failed, entries, _ = _walk(program, tmp_path, slots, 0, full)
    assert failed == 1 and len(entries) == 1024
