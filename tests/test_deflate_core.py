"""The encoder of libgfdeflate.so on the host: genefuserust_amd/scan_csrc/gf_df_core.h, the very text the kernels run,
compiled with g++ under AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone program
(tests/cpp/test_deflate_core.cpp) and held to independent decoders: every text of tests/deflate_cases.py at every size
parses as one BGZF member (bgzf_members.walk_model), inflates under zlib to the text, carries the right CRC-32, ISIZE
and BSIZE and is never longer than a stored member; FASTQ text compresses at least as well as Huffman coding alone, and
random bytes come out stored; the match at the window's edge and what each text made for a limit reaches are read off the
members' own tokens and headers.  Nothing loaded into Python runs under a sanitizer."""
import os
import subprocess
import zlib

import pytest

from genefuserust_amd import deflate   # the feature these tests are for
from tests import bgzf_members as bm
from tests import deflate_cases as dc
from tests import huffman_model as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("deflate_core") / "test_deflate_core")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_deflate_core.cpp")], check=True)
    return exe


def run(program, tmp_path, jobs):
    """The program's answers, a list of token lists; it must end clean under the sanitizers."""
    (tmp_path / "jobs").write_text("".join(j + "\n" for j in jobs))
    done = subprocess.run([program, str(tmp_path / "jobs"), str(tmp_path / "answers")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    out = [line.split() for line in (tmp_path / "answers").read_text().splitlines()]
    assert len(out) == len(jobs)
    return out


@pytest.fixture(scope="module")
def members(program, tmp_path_factory):
    """{(name, size): (text, member, kind)}: every case through the program, once."""
    tmp = tmp_path_factory.mktemp("deflate_members")
    cases = dc.cases()
    jobs = []
    for k, (_, _, text) in enumerate(cases):
        (tmp / ("t%d" % k)).write_bytes(text)
        jobs.append("member %s %s" % (tmp / ("t%d" % k), tmp / ("m%d" % k)))
    out = {}
    for k, ((name, size, text), answer) in enumerate(zip(cases, run(program, tmp, jobs))):
        member = (tmp / ("m%d" % k)).read_bytes()
        assert len(member) == int(answer[0])
        out[name, size] = (text, member, int(answer[1]))
    return out


def test_every_member_reads_back_under_independent_decoders(members):
    assert len(members) == 14 * len(dc.SIZES)
    kinds = set()
    for (name, size), (text, member, kind) in members.items():
        assert len(text) == size
        btype = dc.check_member(member, text)
        assert (btype, kind) in ((0, dc.STORED), (2, dc.DYNAMIC)), (name, size)
        if kind == dc.STORED:
            assert len(member) == size + dc.STORED_OVER
        kinds.add(kind)
    assert kinds == {dc.STORED, dc.DYNAMIC}


def test_quality_floor(members):
    """FASTQ text is not stored and takes at most 1.10 x what Huffman coding alone takes, + 256 bytes: matching must not
    make things worse.  Random bytes come out stored."""
    seen = 0
    for (name, size), (text, member, kind) in members.items():
        if name in ("fastq", "binned") and size >= 4096:
            payload = len(member) - 26
            huffman = len(bm.raw_deflate(text, 1, zlib.Z_HUFFMAN_ONLY))
            print(name, size, "payload", payload, "huffman only", huffman, "level 1", len(bm.raw_deflate(text, 1)))
            assert kind == dc.DYNAMIC, (name, size)
            assert payload <= 1.10 * huffman + 256, (name, size, payload, huffman)
            seen += 1
        if name == "random":
            assert kind == dc.STORED, size
    assert seen == 6
    # the runs and the repeats are found at all: a text of one value, of period 2 and 3 shrink a hundredfold
    for name in ("one_byte_value", "period_2", "period_3", "all_values"):
        assert len(members[name, 65280][1]) < 65280 // 100, name
    # chained matches of 258: 5000 bytes of one value take some twenty tokens
    assert members["chained_258", 65280][2] == dc.DYNAMIC and len(members["chained_258", 65280][1]) < 2000


def positions(tokens):
    """[(where the token starts in the text, token)]"""
    out, pos = [], 0
    for t in tokens:
        out.append((pos, t))
        pos += t[0] if isinstance(t, tuple) else 1
    return out


def test_a_match_reaches_distance_32768_and_no_further(program, tmp_path):
    """``window_edge``: a 64-byte motif recurs at distance 32768 and is one match of exactly that distance; another
    recurs at 32769 and is not copied from there.  Read off the member's own tokens, so nothing but the match passes:
    the ``motif_32768`` text this test used has no match at all (its filler overwrites the table), and its two members
    differed by their histograms alone.  The control has the near copy in reverse order: the same histogram, no copy."""
    near, control = dc.window_edge_member(0), dc.window_edge_member(0, reverse_the_near_copy=True)
    assert near == dc.texts()["window_edge"][:dc.TEXT] and sorted(near) == sorted(control)
    (tmp_path / "near").write_bytes(near)
    (tmp_path / "control").write_bytes(control)
    got = run(program, tmp_path, ["member %s %s" % (tmp_path / n, tmp_path / (n + ".gz")) for n in ("near", "control")])
    m_near, m_control = (tmp_path / "near.gz").read_bytes(), (tmp_path / "control.gz").read_bytes()
    assert dc.check_member(m_near, near) == 2 and dc.check_member(m_control, control) == 2
    assert int(got[0][1]) == int(got[1][1]) == dc.DYNAMIC
    tokens, tokens_control = bm.tokens_of(m_near[18:-8])[3], bm.tokens_of(m_control[18:-8])[3]
    assert bm.replay(tokens) == near and bm.replay(tokens_control) == control
    a, b = dc.WINDOW_EDGE_AT
    # the motif at 32768: one match, from its first byte, as long as the two places agree (the filler behind agrees too)
    agree = next(n for n in range(259) if n == 258 or near[a + n] != near[a + 32768 + n])
    assert agree >= 64
    assert dict(positions(tokens))[a + 32768] == (agree, 32768)
    # nothing reaches farther, and the motif at 32769 comes out as literals or nearer matches
    assert max(t[1] for t in tokens if isinstance(t, tuple)) == 32768
    second = [(pos, t) for pos, t in positions(tokens)
              if pos < b + 32769 + 64 and pos + (t[0] if isinstance(t, tuple) else 1) > b + 32769]
    assert second and all(not isinstance(t, tuple) or t[1] < 32768 for _, t in second), second
    assert near[b:b + 64] == near[b + 32769:b + 32769 + 64]                    # (it is there to be copied)
    # the control: no match at the edge, the 64 bytes are literals, and the member is longer
    assert max(t[1] for t in tokens_control if isinstance(t, tuple)) < 32768
    at = dict(positions(tokens_control))
    assert all(at[a + 32768 + k] == control[a + 32768 + k] for k in range(64))
    assert len(m_control) > len(m_near) + 20


NEW_TEXTS = {"window_edge": dc.window_edge_member, "deep_literals": dc.deep_literals_member,
             "deep_distances": dc.deep_distances_member, "deep_code_lengths": dc.deep_code_lengths_member,
             "every_symbol": dc.every_symbol_member}


def taken_apart(member):
    """(literal/length lengths [286], distance lengths [30], code-length lengths, tokens, literal/length counts, distance
    counts) of a dynamic member."""
    lit, dist, cl, tokens = bm.tokens_of(member[18:-8])
    lf, df = bm.token_symbols(tokens)
    return lit + [0] * (286 - len(lit)), dist + [0] * (30 - len(dist)), cl, tokens, lf, df


def test_what_every_text_reaches(members, program, tmp_path):
    """The coverage pin: what each text of the code-length limits and the window edge is there for, asserted on its
    members' own headers and tokens (both members of each), so that a text that stops reaching its branch fails here.
    And for every dynamic member of every case: the tokens replay to the text, and gf_df_plan on their histogram gives the
    header's code lengths and the payload's length."""
    todo = [(name, size, text, member) for (name, size), (text, member, kind) in members.items() if kind == dc.DYNAMIC]
    for name, make in NEW_TEXTS.items():
        text = make(1)
        assert dc.texts()[name] == make(0) + text + make(0)[:1]
        (tmp_path / name).write_bytes(text)
        job = "member %s %s" % (tmp_path / name, tmp_path / (name + ".gz"))
        assert run(program, tmp_path, [job])[0][1] == str(dc.DYNAMIC)
        member = (tmp_path / (name + ".gz")).read_bytes()
        assert dc.check_member(member, text) == 2
        todo.append((name, "second", text, member))
    assert len(todo) > 80
    apart, jobs = [], []
    for k, (name, size, text, member) in enumerate(todo):
        apart.append(taken_apart(member))
        assert bm.replay(apart[-1][3]) == text == zlib.decompress(member[18:-8], -15), (name, size)
        (tmp_path / ("h%d" % k)).write_text(" ".join(str(c) for c in apart[-1][4] + apart[-1][5]))
        jobs.append("plan %s" % (tmp_path / ("h%d" % k)))
    reached = {}
    plans = run(program, tmp_path, jobs)
    for (name, size, text, member), (lit, dist, cl, tokens, lf, df), plan in zip(todo, apart, plans):
        plan = [int(x) for x in plan]
        assert plan[:316] == lit + dist and plan[316:335] == cl, (name, size)
        assert (plan[356] + 7) // 8 == len(member) - 26, (name, size)
        matches = [t for t in tokens if isinstance(t, tuple)]
        assert all(t[0] >= 5 for t in matches)           # gf_df_min_len: lengths 3 and 4 are never taken
        if size in (dc.TEXT, "second"):
            hdist = max(s + 1 for s in range(30) if dist[s] or s == 0)
            cl_counts = [(lit + dist[:hdist]).count(l) for l in range(19)]
            reached[name, size] = dict(
                depths=(hm.huffman_depth(lf), hm.huffman_depth(df), hm.huffman_depth(cl_counts)),
                longest=(max(lit), max(dist), max(cl)), lengths={t[0] for t in matches},
                distances={t[1] for t in matches}, symbols={s for s in range(30) if df[s]},
                widest=max([dist[s] + bm.DIST_EXTRA[s] for s in range(30) if df[s]], default=0))
    for name in NEW_TEXTS:
        for size in (dc.TEXT, "second"):
            r = reached[name, size]
            print(name, size, "unrestricted depths", r["depths"], "longest codes", r["longest"], "distance symbols",
                  len(r["symbols"]), "lengths", len(r["lengths"]), "widest distance unit", r["widest"])
            if name == "window_edge":
                assert max(r["distances"]) == 32768
            if name == "deep_literals":                  # the limit binds by three levels and more
                assert r["depths"][0] >= 18 and r["longest"][0] == 15
            if name == "deep_distances":                 # and a 15-bit distance code with 13 extra bits: 28 bits
                assert r["depths"][1] > 15 and r["longest"][1] == 15 and r["widest"] == 28
            if name in ("deep_distances", "deep_code_lengths"):
                assert r["depths"][2] > 7 and r["longest"][2] == 7
            if name == "every_symbol":
                assert r["lengths"] == set(range(5, 259)) and r["symbols"] == set(range(30))
    # the texts from before reach none of it: the limits and the edge are these texts' alone
    for name in ("fastq", "binned", "motif_32768", "chained_258"):
        r = reached[name, dc.TEXT]
        assert r["depths"][0] <= 16 and r["depths"][1] <= 15 and max(r["distances"], default=0) < 32768


def test_the_program_is_the_library(members):
    """gf_df_member_host (the library's host build of the same header) gives the program's bytes."""
    for (name, size), (text, member, _) in members.items():
        if size in (1, 17, 259, 4096, 65280):
            assert deflate.deflate_member_host(text) == member, (name, size)


def test_symbols_and_minimum_lengths(program, tmp_path):
    """Every length and a sweep of distances land on the symbol, the extra bits and the value of RFC 1951's tables."""
    lengths = list(range(3, 259))
    dists = sorted(set(list(range(1, 600)) + [d + k for d in bm.DIST_BASE for k in (-1, 0, 1) if 1 <= d + k <= 32768]
                       + [32767, 32768]))
    got = run(program, tmp_path, ["len %d" % (n - 3) for n in lengths] + ["dist %d" % (d - 1) for d in dists]
              + ["minlen %d" % d for d in dists])
    for n, g in zip(lengths, got):
        k = 28 if n == 258 else max(i for i in range(28) if bm.LEN_BASE[i] <= n)
        assert [int(x) for x in g] == [k, bm.LEN_EXTRA[k], n - bm.LEN_BASE[k]], n
    for d, g in zip(dists, got[len(lengths):]):
        k = max(i for i in range(30) if bm.DIST_BASE[i] <= d)
        assert [int(x) for x in g] == [k, bm.DIST_EXTRA[k], d - bm.DIST_BASE[k]], d
    floors = [int(g[0]) for g in got[len(lengths) + len(dists):]]
    assert floors == sorted(floors) and floors[0] >= 3 and floors[-1] <= 258      # farther costs more, never less
    # a far match must pay for its 13 extra bits against literals of 2 bits
    assert floors[-1] * 2 >= 13 + 10
