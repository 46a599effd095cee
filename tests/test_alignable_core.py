"""The arithmetic of libgfalign.so on the host: genefuserust_amd/scan_csrc/gf_al_core.h, the very text the kernels run,
compiled with g++ under AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone program
(tests/cpp/test_alignable_core.cpp) and held to the brute-force model of the predicate (tests/alignable_model.py)."""
import os
import subprocess

import numpy as np
import pytest

from genefuserust_amd.fusion_mapper import reverse_complement
from tests.alignable_model import K, LIMIT, alignable, uncovered
from tests.helpers import rand_seq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEPARATOR = b"\0"


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("alignable_core") / "test_alignable_core")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_alignable_core.cpp")],
                   check=True)
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


def mutate(rng, s: bytes, n: int, alphabet: bytes = b"ACGT") -> bytes:
    out = bytearray(s)
    for i in rng.integers(0, len(s), n).tolist():
        out[i] = alphabet[(alphabet.index(out[i]) + 1) % 4] if out[i] in alphabet else alphabet[0]
    return bytes(out)


def flip(s: bytes) -> bytes:
    """Every base another one."""
    return bytes(ord("A") if b != ord("A") else ord("C") for b in s)


def diagonal_jobs():
    """[(strand, text, p)]: a few hundred random diagonals, reads of 16, 25, 26 and 4096 bases among them, the text in
    mixed case and with bytes outside ACGT, substitutions 0 .. 12 and in runs at either end."""
    rng = np.random.default_rng(21)
    jobs = []
    for L in [16, 25, 26, 4096] + rng.integers(16, 400, 60).tolist():
        for _ in range(2 if L == 4096 else 4):
            text = bytearray(rand_seq(rng, L + int(rng.integers(0, 80))))
            p = int(rng.integers(0, len(text) - L + 1))
            s = bytes(text[p:p + L])
            for i in rng.integers(0, len(text), int(rng.integers(0, 3))).tolist():
                text[i] = ord("N")
            if rng.integers(0, 2):
                lo = int(rng.integers(0, len(text)))
                text[lo:lo + 40] = bytes(text[lo:lo + 40]).lower()
            kind = int(rng.integers(0, 4))
            if kind == 0:
                s = mutate(rng, s, int(rng.integers(0, 13)))
            elif kind == 1:      # a run of k substitutions at the head or the tail: the LIMIT edge
                k = min(L, int(rng.integers(7, 13)))
                s = flip(s[:k]) + s[k:] if rng.integers(0, 2) else s[:L - k] + flip(s[L - k:])
            elif kind == 2:
                s = s[:L // 2] + b"N" + s[L // 2 + 1:]
            jobs.append((s, bytes(text), p))
            jobs.append((s, bytes(text), int(rng.integers(0, len(text) - L + 1))))   # and an unrelated diagonal
    return jobs


def test_diagonals_against_the_model(program, tmp_path):
    jobs = diagonal_jobs()
    assert len(jobs) >= 300 and {16, 25, 26, 4096} <= {len(s) for s, _, _ in jobs}
    got = run(program, tmp_path, ["diag %s %s %d" % (hx(s), hx(t), p) for s, t, p in jobs])
    seen = set()
    for (s, t, p), (ok, u) in zip(jobs, got):
        want = uncovered(s, t.upper(), p)
        assert int(u) == want and int(ok) == (want < LIMIT), (len(s), p)
        seen.add(want < LIMIT)
    assert seen == {True, False}
    # the boundary itself: 9 and 10 uncovered positions at either end and in the middle
    text = rand_seq(np.random.default_rng(2), 120)
    bad, edge = flip(text), []
    for k in (9, 10):
        edge += [(bad[:k] + text[k:100], text, 0), (text[:100 - k] + bad[100 - k:100], text, 0),
                 (text[:40] + bad[40:41] + text[41:40 + k] + bad[40 + k:41 + k] + text[41 + k:100], text, 0)]
    got = run(program, tmp_path, ["diag %s %s %d" % (hx(s), hx(t), p) for s, t, p in edge])
    assert [[int(x) for x in g] for g in got] == [[1, 9], [1, 9], [0, 10], [0, 10], [0, 10], [0, 11]]


def test_refused_diagonals(program, tmp_path):
    text = rand_seq(np.random.default_rng(3), 100)
    s = text[10:60]
    jobs = [(s, text, -1), (s, text, 51), (s, text, 50), (text[:15], text, 0), (s, text[:30] + SEPARATOR + text[31:], 10),
            (s, text[:9] + SEPARATOR + text[10:60] + SEPARATOR + text[61:], 10), (b"", text, 0), (text + b"A", text, 0)]
    got = run(program, tmp_path, ["diag %s %s %d" % (hx(a), hx(t), p) for a, t, p in jobs])
    assert [[int(x) for x in g] for g in got] == [[0, -1], [0, -1], [0, 50], [0, -1], [0, -1], [1, 0], [0, -1], [0, -1]]


def test_strands_and_keys(program, tmp_path):
    rng = np.random.default_rng(5)
    reads = [rand_seq(rng, n) for n in (1, 15, 16, 17, 64, 300)] + [b"ACGTacgtNnXx\0\xff-*", b""]
    reads.append(bytes(rng.integers(0, 256, 200, dtype=np.uint8)))
    got = run(program, tmp_path, ["strands %s" % hx(r) for r in reads])
    assert [g[0] for g in got] == [hx(reverse_complement(r)) for r in reads]
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    strings = [rand_seq(rng, 16), rand_seq(rng, 15), rand_seq(rng, 200), b"A" * 40, b"T" * 16,
               rand_seq(rng, 30) + b"N" + rand_seq(rng, 30), rand_seq(rng, 40).lower(), rand_seq(rng, 4096)]
    got = run(program, tmp_path, ["keys %s" % hx(s) for s in strings])
    for s, g in zip(strings, got):
        want = []
        for j in range(len(s) - K + 1):
            w = s[j:j + K]
            want.append(sum(code[b] << (2 * (K - 1 - i)) for i, b in enumerate(w)) if all(b in code for b in w) else -1)
        assert [int(x) for x in g[:-1]] == want and g[-1] == "ok", len(s)


def piece_of(contigs):
    return SEPARATOR.join(contigs)


def test_a_read_against_a_piece(program, tmp_path):
    """The scan of a piece as the kernel does it — seeds, the first window of an exact run only, the diagonal — against
    the model, the piece's contigs being its reference: reads drawn from it with 0 .. 12 substitutions, either strand,
    reads across two contigs of the piece, a tandem repeat, and reads of 16, 25, 26 and 4096 bases."""
    rng = np.random.default_rng(8)
    unit = rand_seq(rng, 23)
    contigs = [rand_seq(rng, 700), (unit * 30)[:600], rand_seq(rng, 5000).lower(), rand_seq(rng, 20)]
    contigs[0] = contigs[0][:300] + b"N" * 12 + contigs[0][312:]
    reference = {str(i): c for i, c in enumerate(contigs)}
    text = piece_of(contigs)
    flat = b"".join(contigs).upper()
    reads = []
    for L in [16, 25, 26, 4096] + rng.integers(16, 320, 70).tolist():
        p = int(rng.integers(0, len(flat) - L + 1)) if L < 4096 else 1300 + int(rng.integers(0, 900))
        r = mutate(rng, flat[p:p + L], int(rng.integers(0, 13)) if rng.integers(0, 3) else 0)
        reads.append(reverse_complement(r) if rng.integers(0, 2) else r)
    reads += [flat[690:730], flat[1290:1330], contigs[3], rand_seq(rng, 100), unit * 4, (unit * 4)[5:70]]
    got = run(program, tmp_path, ["read %s %s" % (hx(r), hx(text)) for r in reads])
    want = [alignable(reference, r) for r in reads]
    assert [int(g[0]) == 1 for g in got] == want
    assert 10 < sum(want) < len(want) - 10
