"""The arithmetic of libgfreport.so on the host: genefuserust_amd/scan_csrc/gf_rp_core.h, the very text the kernels run,
compiled with g++ under AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone program
(tests/cpp/test_report_core.cpp) and held to gf_edit_distance, gf_readmatch_filter and FusionResult.calc_ed /
adjust_fusion_break of the Python mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from genefuserust_amd import GenePos, ReadMatch, _lib
from genefuserust_amd.fusion_mapper import edit_distance
from genefuserust_amd.fusion_result import FusionResult
from tests.helpers import rand_seq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, OUT_OF_DOMAIN = 0, 1


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("report_core") / "test_report_core")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_report_core.cpp")], check=True)
    return exe


def hx(b: bytes) -> str:
    return b.hex() or "-"


def run(program, tmp_path, jobs):
    """The program's answers, a list of int lists; it must end clean under the sanitizers."""
    (tmp_path / "jobs").write_text("".join(j + "\n" for j in jobs))
    done = subprocess.run([program, str(tmp_path / "jobs"), str(tmp_path / "answers")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    out = [[int(x) for x in line.split()] for line in (tmp_path / "answers").read_text().splitlines()]
    assert len(out) == len(jobs)
    return out


def test_edit_distance(program, tmp_path):
    rng = np.random.default_rng(3)
    pairs = []
    for m in (0, 1, 19, 20, 21, 63, 64, 65, 127, 128, 129, 250, 4096):
        p = rand_seq(rng, m)
        texts = [p, b"", rand_seq(rng, m), rand_seq(rng, m // 2), rand_seq(rng, m + 1 + m // 3), p[:m // 2], p + p[:7]]
        if m:
            first, last = bytearray(p), bytearray(p)
            first[0] = ord("A") if p[0] != ord("A") else ord("C")
            last[-1] = ord("A") if p[-1] != ord("A") else ord("C")
            texts += [bytes(first), bytes(last), b"G" + p, b"G" + p[:-1], p[1:], p[1:] + b"T",   # an insertion shifts all
                      p.lower(), p[:m // 2] + b"N" + p[m // 2 + 1:], p[:m // 2].lower() + p[m // 2:],
                      bytes(rng.integers(0, 256, m, dtype=np.uint8))]
        pairs += [(p, t) for t in texts] + [(t, p) for t in texts[1:4]]
    got = run(program, tmp_path, ["ed %s %s" % (hx(a), hx(b)) for a, b in pairs])
    for (a, b), (d,) in zip(pairs, got):
        assert d == edit_distance(a, b), (len(a), len(b))


def filter_cases():
    """[(seq, ReadMatch fields (break, ld, rd, lp, rp, lcontig, rcontig), threshold)] on every boundary."""
    rng = np.random.default_rng(5)
    varied = rand_seq(rng, 60)

    def runs(n_unequal, n):     # n bases with exactly n_unequal unequal neighbours
        s = bytearray(b"A" * n)
        for k in range(n_unequal):
            s[k + 1:] = bytes([b"AC"[(k + 1) & 1]]) * (n - k - 1)
        assert sum(s[i] != s[i + 1] for i in range(n - 1)) == n_unequal
        return bytes(s)
    out = []
    for left in (19, 20):
        out.append((varied[:left] + varied[:30], (left - 1, 0, 0, 100, 900, 0, 1), 50))
        out.append((varied[:30] + varied[:left], (29, 0, 0, 100, 900, 0, 1), 50))
    for u in (6, 7):
        out.append((runs(u, 30) + varied[:30], (29, 0, 0, 100, 900, 0, 1), 50))
        out.append((varied[:30] + runs(u, 30), (29, 0, 0, 100, 900, 0, 1), 50))
    for ld, rd in ((4, 0), (2, 2), (5, 0), (2, 3), (0, 5)):
        out.append((varied, (29, ld, rd, 100, 900, 0, 1), 50))
    for lp, rp in ((100, 149), (100, 150), (149, 100), (150, 100), (-100, -149), (-100, -150), (-20, 29), (-20, 30)):
        out.append((varied, (29, 0, 0, lp, rp, 1, 1), 50))
        out.append((varied, (29, 0, 0, lp, rp, 0, 1), 50))
    out.append((varied, (29, 0, 0, 500, 500, 0, 1), 50))     # different contigs at distance 0
    out.append((varied, (29, 3, 3, 500, 500, 1, 1), 50))     # the distance test comes before the deletion test
    out.append((varied[:10] + varied, (9, 3, 3, 500, 500, 1, 1), 50))   # and complexity before both
    out.append((varied, (29, 0, 0, 100, 120, 1, 1), 0))
    out.append((varied, (-1, 0, 0, 100, 900, 0, 1), 50))     # an empty left side: low complexity
    out.append((varied, (59, 0, 0, 100, 900, 0, 1), 50))     # an empty right side
    out.append((varied, (-2, 0, 0, 100, 900, 0, 1), 50))     # outside the read
    out.append((varied, (60, 0, 0, 100, 900, 0, 1), 50))
    out.append((b"", (-1, 0, 0, 100, 900, 0, 1), 50))
    return out


def host_filter_reason(seq, f, thr):
    """gf_readmatch_filter; its GF_ERR_ARG for a break outside the read is the core's -1."""
    rm = _lib.GfReadMatch(f[0], 0, f[1], f[2], f[3], f[4], f[5], f[6])
    why = _lib.lib().gf_readmatch_filter(C.byref(rm), seq, len(seq), thr)
    return -1 if why == _lib.GF_ERR_ARG else why


def test_filter(program, tmp_path):
    cases = filter_cases()
    got = run(program, tmp_path, ["filter %s %s %d" % (hx(s), " ".join(str(v) for v in f), thr) for s, f, thr in cases])
    want = [host_filter_reason(s, f, thr) for s, f, thr in cases]
    assert [g[0] for g in got] == want
    assert set(want) == {-1, 0, 1, 2, 3}


def adjust_cases():
    """[(read, read_break, left reference, right reference)]"""
    rng = np.random.default_rng(7)
    out = []
    for brk in (59, 60, 61, 62, 63, 64, 65, 66, 123, 124, 125, 126, 127, 128, 129, 130):   # break + shift + 1 over 64, 128
        lref, rref = rand_seq(rng, brk + 8), rand_seq(rng, 100)
        read = bytearray(lref[-(brk + 1):] + rref[:90])
        read[5], read[brk + 40] = ord("N"), ord("a")
        out.append((bytes(read), brk + int(rng.integers(-2, 3)), lref, rref))
    # a tie between shifts: a junction inside a run of one base fits every shift as well as the next; the earliest wins
    left, right = rand_seq(rng, 40), rand_seq(rng, 40)
    out.append((left + b"G" * 12 + right, 45, rand_seq(rng, 10) + left + b"G" * 6, b"G" * 6 + right))
    out.append((b"A" * 80, 40, b"A" * 50, b"A" * 50))
    read = rand_seq(rng, 100)
    out.append((read, 50, b"", read[51:]))                        # an empty left reference
    out.append((read, 50, read[:51], b""))                        # an empty right reference
    out.append((read, 50, b"", b""))
    out.append((read, 50, read[30:51], read[51:70]))              # references shorter than the read's parts
    out.append((read, 50, read[45:51], read[51:54]))              # and shorter than the window
    out.append((read, 50, rand_seq(rng, 300), rand_seq(rng, 300)))   # longer, and unrelated
    long_read = rand_seq(rng, 4096)
    out.append((long_read, 2000, long_read[:2001], long_read[2001:]))
    out.append((long_read, 4091, rand_seq(rng, 4096), rand_seq(rng, 3)))
    for brk in (-5, -1, 0, 1, 2, 3, 94, 95, 96, 97, 99, 100, 120):   # 3 .. len - 5 is the domain
        out.append((read, brk, read[:40], read[60:]))
    return out


def host_adjust(read, brk, lref, rref):
    fr = FusionResult(m_left_ref=lref, m_right_ref=rref)
    m = ReadMatch(read, brk, GenePos(0, 1000), GenePos(1, 2000), 1, 77, 88)
    fr.add_match(m)
    fr.adjust_fusion_break()
    a = fr.m_matches[0]
    return [a.m_read_break - brk, a.m_left_distance, a.m_right_distance]


def test_adjust(program, tmp_path):
    cases = adjust_cases()
    got = run(program, tmp_path, ["adjust %s %d %s %s" % (hx(r), b, hx(lr), hx(rr)) for r, b, lr, rr in cases])
    n_in = 0
    for (read, brk, lref, rref), g in zip(cases, got):
        if 3 <= brk <= len(read) - 5:
            assert g == host_adjust(read, brk, lref, rref) + [OK], (len(read), brk, len(lref), len(rref))
            n_in += 1
        else:
            assert g == [0, 0, 0, OUT_OF_DOMAIN], (len(read), brk)
    assert n_in >= 28
    # the ties are ties: the earliest of several equally good shifts was chosen
    fr = FusionResult(m_left_ref=cases[17][2], m_right_ref=cases[17][3])
    totals = [fr.calc_ed(ReadMatch(cases[17][0], cases[17][1], GenePos(0, 0), GenePos(0, 0), 0, 0, 0), s)[0]
              for s in range(-3, 4)]
    assert totals.count(min(totals)) > 1 and got[17][0] == totals.index(min(totals)) - 3
