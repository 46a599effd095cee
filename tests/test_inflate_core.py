"""The DEFLATE decoder of libgfinflate.so on the host: genefuserust_amd/scan_csrc/gf_if_core.h, the very text the kernels
run, compiled with g++ under AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone program
(tests/cpp/test_inflate_core.cpp) and held to zlib on every block kind, on members zlib cannot emit, and on every way a
member can be wrong."""
import gzip
import os
import subprocess
import zlib

import numpy as np
import pytest

from tests import bgzf_members as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inflate_core") / "test_inflate_core")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_inflate_core.cpp")], check=True)
    return exe


def run(program, tmp_path, comp: bytes, table: np.ndarray, out_cap: int):
    """(output bytes, statuses) of the host program; it must end clean under the sanitizers."""
    (tmp_path / "comp").write_bytes(comp)
    (tmp_path / "table").write_bytes(np.ascontiguousarray(table, dtype=np.int64).tobytes())
    done = subprocess.run([program, str(tmp_path / "comp"), str(tmp_path / "table"), str(out_cap), str(tmp_path / "out"),
                           str(tmp_path / "status")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    out = (tmp_path / "out").read_bytes()
    assert len(out) == out_cap
    return out, np.frombuffer((tmp_path / "status").read_bytes(), dtype=np.int32)


def check_good(program, tmp_path, cases):
    """``cases`` [(name, text, member)], back to back at odd offsets with sentinels between their texts."""
    for name, text, m in cases:
        assert gzip.decompress(m) == text, name
    comp, table, need = bm.table_of([m for _, _, m in cases], text_gap=3, comp_gap=1, text_base=5)
    out, status = run(program, tmp_path, comp, table, need + 7)
    assert status.tolist() == [0] * len(cases), [(c[0], int(s)) for c, s in zip(cases, status) if s]
    expect = bytearray([SENTINEL]) * (need + 7)
    for (name, text, _), row in zip(cases, table):
        expect[row[2]:row[2] + row[3]] = text
    for (name, text, _), row in zip(cases, table):
        assert out[row[2]:row[2] + row[3]] == text, name
    assert out == bytes(expect)


def test_block_kinds_of_zlib(program, tmp_path):
    cases = bm.kinds()
    by_name = {name: bm.parts(m)[0] for name, _, m in cases}
    # the kinds are what the names say
    assert bm.block_kinds(by_name["stored_level0"]) == (0, 0)
    assert bm.block_kinds(by_name["stored_random"])[0] == 0
    for name in ("fixed", "one_byte", "empty"):
        assert bm.block_kinds(by_name[name])[0] == 1, name
    for name in ("level1", "level6", "level9", "huffman_only", "rle", "all_a"):
        assert bm.block_kinds(by_name[name])[0] == 2, name
    assert bm.block_kinds(by_name["all_a"]) == (2, 1)          # one block; the FASTQ members take several
    assert bm.block_kinds(by_name["huffman_only"])[1] == 0 and bm.block_kinds(by_name["rle"])[1] == 0
    assert len(dict((n, m) for n, _, m in cases)["all_a"]) == 106
    check_good(program, tmp_path, cases)


def test_periodic_texts_and_a_full_member(program, tmp_path):
    cases = [("period_%d" % p, bm.periodic(p), bm.member(bm.periodic(p))) for p in bm.PERIODS]
    full = bm.fastq_text(65536, seed=4)
    cases.append(("isize_65536", full, bm.member(full)))
    check_good(program, tmp_path, cases)


def test_members_zlib_cannot_emit(program, tmp_path):
    check_good(program, tmp_path, bm.hand_assembled() + bm.valid_dynamic())


def test_codes_at_their_limits(program, tmp_path):
    """``deep_codes``: literal/length and distance codes of 13, 14 and 15 bits in use, a code-length code of 5 to 7
    bits, the repeat codes at their largest counts and across the two alphabets, length 258 both ways, distance 32768
    under a 15-bit code — by hand, by this project's encoder on the texts made for its limits, and by zlib on the same
    texts.  What the hand-made blocks hold is read off them first, by a parser of its own."""
    lit, dist, cl, tokens = bm.tokens_of(bm.deep_dynamic()[-2][2])
    assert {13, 14, 15} <= set(lit) and {13, 14, 15} <= set(dist) and {2, 3, 4, 5, 6, 7} == set(cl)
    assert tokens[-1] == (258, 32768) and (258, 32768) in tokens[:-1] and (3, 16385 + 8191) in tokens
    lit, dist, cl, tokens = bm.tokens_of(bm.deep_dynamic()[-1][2])
    assert lit[138:145] == [3] * 7 and lit[145:256] == [0] * 111 and lit[257:] + dist[:5] == [5] * 7
    cases = bm.deep_codes()
    names = [c[0] for c in cases]
    assert len(cases) == 28 and "codes_of_13_14_15_bits_and_258_by_284" in names      # zlib takes 258 = 227 + 31
    deep = {c[0]: bm.tokens_of(bm.parts(c[2])[0]) for c in cases if c[0].endswith("_own")}
    assert max(deep["deep_literals_0_own"][0]) == 15 and max(deep["deep_distances_1_own"][1]) == 15
    assert max(deep["deep_code_lengths_0_own"][2]) == 7 and (201, 32768) in deep["window_edge_0_own"][3]
    check_good(program, tmp_path, cases)


def test_malformed_members(program, tmp_path):
    bad = bm.malformed()
    good_text = bm.fastq_text(5000, seed=8)
    good = bm.member(good_text)
    members, names, want = [], [], []
    for name, m, status in bad:      # a good member between any two bad ones
        members += [m, good]
        names += [name, "good"]
        want += [status, 0]
    comp, table, need = bm.table_of(members, text_gap=3, comp_gap=1, text_base=5)
    out, status = run(program, tmp_path, comp, table, need + 7)
    assert all(s != 0 for s, w in zip(status, want) if w), [n for n, s, w in zip(names, status, want) if w and not s]
    assert status.tolist() == want, [(n, int(s), w) for n, s, w in zip(names, status, want) if s != w]
    expect = bytearray([SENTINEL]) * (need + 7)
    for w, row in zip(want, table):
        if w == 0:
            expect[row[2]:row[2] + row[3]] = good_text
    assert out == bytes(expect)      # the bad members' own ranges too: nothing is written for them
    # every way of the decoder's list occurs
    assert set(want) >= set(range(1, 16)) | {bm.BAD_CODE, bm.TRAILING}


def test_rows_that_point_outside(program, tmp_path):
    text = bm.fastq_text(1000, seed=2)
    comp, table, need = bm.table_of([bm.member(text)] * 8)
    table[1, 0] = len(comp) - 3                 # payload past the end of the compressed bytes
    table[2, 0] = -1
    table[3, 2] = need - 999                    # text past the end of the output
    table[4, 2] = -1
    table[5, 3] = bm.MAX_TEXT + 1
    table[6, 1] = bm.MAX_TEXT + 1
    out, status = run(program, tmp_path, comp, table, need)
    assert status.tolist() == [0] + [bm.BAD_ROW] * 6 + [0]
    assert out[:1000] == text and out[7000:8000] == text and set(out[1000:7000]) == {SENTINEL}


def test_crc_join_is_zlibs_crc(program, tmp_path):
    """The CRC is taken in 64 pieces and joined: lengths around the piece boundaries, each with the right and a wrong
    CRC."""
    rng = np.random.default_rng(12)
    texts = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in (1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097)]
    members = []
    for t in texts:
        members += [bm.member(t), bm.wrap(bm.raw_deflate(t), zlib.crc32(t) ^ 0x80000000, len(t))]
    comp, table, need = bm.table_of(members)
    _, status = run(program, tmp_path, comp, table, need)
    assert status.tolist() == [0, bm.CRC] * len(texts)
