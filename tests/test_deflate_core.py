"""The encoder of libgfdeflate.so on the host: genefuserust_amd/scan_csrc/gf_df_core.h, the very text the kernels run,
compiled with g++ under AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone program
(tests/cpp/test_deflate_core.cpp) and held to independent decoders: every text of tests/deflate_cases.py at every size
parses as one BGZF member (bgzf_members.walk_model), inflates under zlib to the text, carries the right CRC-32, ISIZE
and BSIZE and is never longer than a stored member; FASTQ text compresses at least as well as Huffman coding alone, and
random bytes come out stored.  Nothing loaded into Python runs under a sanitizer."""
import os
import subprocess
import zlib

import pytest

from genefuserust_amd import deflate   # the feature these tests are for
from tests import bgzf_members as bm
from tests import deflate_cases as dc

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
    assert len(members) == 9 * len(dc.SIZES)
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


def test_a_match_reaches_distance_32768_and_no_further(program, tmp_path):
    """The 64-byte motif recurs at distance 32768 (within reach: its second copy costs a match) and at 32769 (out of
    reach: its second copy costs literals).  Moving the near one out of reach too makes the member longer."""
    text = bytearray(dc.texts()["motif_32768"][:dc.TEXT])
    (tmp_path / "near").write_bytes(bytes(text))
    far = bytearray(text)
    far[100 + 32768:100 + 32768 + 64] = bytes(b ^ 0x55 for b in far[100 + 32768:100 + 32768 + 64])   # no copy any more
    (tmp_path / "far").write_bytes(bytes(far))
    got = run(program, tmp_path, ["member %s %s" % (tmp_path / n, tmp_path / (n + ".gz")) for n in ("near", "far")])
    near, gone = (tmp_path / "near.gz").read_bytes(), (tmp_path / "far.gz").read_bytes()
    assert dc.check_member(near, bytes(text)) == 2 and dc.check_member(gone, bytes(far)) == 2
    assert int(got[0][1]) == int(got[1][1]) == dc.DYNAMIC
    assert len(near) + 20 < len(gone)


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
