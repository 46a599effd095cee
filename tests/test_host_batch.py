"""genefuserust_amd/csrc/gf_host_batch.h on the host: the one check of a pack's offsets and the two layouts of the
host-buffer calls (the staged batch in a lane's or a stream slot's device arena, the pinned block of a zero-copy
call), compiled with g++ under AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone program
(tests/cpp/test_host_batch.cpp) and held to a model written here.  The model's arithmetic is a transcription of
gfmatch.hip as it was at commit 8a31298, before the header existed: stage_and_map (check: lines 1404-1414, the al()
sums: 1415-1429), gf_stream_open (2463-2478), zc_submit (sz_*: 1483-1490), gf_stream_submit_packed (chunks and its
capacity test: 2563-2567), gf_compact_workspace_bytes (1198-1202)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_TOO_LONG = 0, -1, -5
MAX_READ_LEN = 4096
SEQMATCH, HIT = 16, 48          # sizeof(gf_seqmatch), sizeof(gf_hit)
READS = (0, 1, 63, 64, 65, 8192, 8193)
BYTES = (0, 1, 15, 16, 17, 255, 256, 4096 * 8193)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_batch") / "test_host_batch")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_host_batch.cpp")], check=True)
    return exe


def run(program, tmp_path, jobs):
    """The program's answers, a list of integer lists; it must end clean under the sanitizers."""
    (tmp_path / "jobs").write_text("".join(j + "\n" for j in jobs))
    done = subprocess.run([program, str(tmp_path / "jobs"), str(tmp_path / "answers")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    out = [[int(x) for x in line.split()] for line in (tmp_path / "answers").read_text().splitlines()]
    assert len(out) == len(jobs)
    return out


# ---- the pack check ------------------------------------------------------------------------------------------------
def model_check(offsets, n, have_reads):
    """8a31298 stage_and_map, lines 1404-1414 (zc_submit 1472-1480 and the two stream submits: the same loop)."""
    if n < 0:
        return [ERR_ARG]
    if n > 0 and offsets is None:
        return [ERR_ARG]
    maxlen = 0
    for r in range(n):
        l = offsets[r + 1] - offsets[r]
        if l < 0:
            return [ERR_ARG]
        maxlen = max(maxlen, l)
    if maxlen > MAX_READ_LEN:
        return [ERR_TOO_LONG]
    b0, b1 = (offsets[0], offsets[n]) if n > 0 else (0, 0)
    if b1 > b0 and not have_reads:
        return [ERR_ARG]
    return [OK, b0, b1, maxlen]


def check_job(offsets, n, have_reads):
    return "check %d %d %s" % (have_reads, n, "null" if offsets is None else " ".join(str(x) for x in offsets))


def pack_cases():
    rng = np.random.default_rng(5)
    cases = [(None, 0, 1), (None, 0, 0), (None, 1, 1), (None, -1, 1), ([0], -3, 1)]
    for n in (0, 1, 2, 64, 65):
        lens = [int(x) for x in rng.integers(0, 300, n)]
        off = [0] + [int(x) for x in np.cumsum(lens)] if n else []
        cases.append((off, n, 1))
        if n == 0:
            continue
        cases.append(([7] * (n + 1), n, 1))                       # all-equal offsets: empty reads
        cases.append(([7] * (n + 1), n, 0))                       # ... need no bases
        cases.append((off, n, 0))                                 # null bases, a span that holds some (or none: n = 1, length 0)
        cases.append(([x + 12345 for x in off], n, 1))            # a non-zero first offset
        cases.append(([x - 77 for x in off], n, 1))               # a negative one
        for at in sorted({0, n // 2, n - 1}):                     # a decrease at the first, a middle, the last position
            bad = list(off)
            for k in range(at + 1, n + 1):
                bad[k] -= lens[at] + 1
            cases.append((bad, n, 1))
        for at in sorted({0, n // 2, n - 1}):
            for length, code in ((MAX_READ_LEN, OK), (MAX_READ_LEN + 1, ERR_TOO_LONG)):
                ls = list(lens)
                ls[at] = length
                cases.append(([0] + [int(x) for x in np.cumsum(ls)], n, 1))
                assert model_check(cases[-1][0], n, 1)[0] == code
        if n >= 2:                                                # too long AND decreasing behind it: the decrease decides
            cases.append(([0, MAX_READ_LEN + 1] + [5] * (n - 1), n, 1))
            assert model_check(cases[-1][0], n, 1) == [ERR_ARG]
    return cases


def test_pack_check_against_the_model(program, tmp_path):
    cases = pack_cases()
    got = run(program, tmp_path, [check_job(*c) for c in cases])
    want = [model_check(*c) for c in cases]
    assert {w[0] for w in want} == {OK, ERR_ARG, ERR_TOO_LONG}
    for c, g, w in zip(cases, got, want):
        assert g == w, (c[1], c[2], (c[0] or [])[:4])


# ---- the staged batch ----------------------------------------------------------------------------------------------
def al(x, a=256):
    return (x + a - 1) & ~(a - 1)


def compact_ws_bytes(n):
    """8a31298 gf_compact_workspace_bytes, lines 1198-1202 (GF_CTILE = 4096, gf_compact_kernels.h:15)."""
    return 0 if n < 0 else 64 + ((n + 4095) // 4096) * (4 + 8) + 16


def model_staged(reads, nbytes, hits_cap):
    """8a31298 stage_and_map, lines 1415-1429 = gf_stream_open, lines 2463-2478 with hits_cap = max_reads."""
    sizes = [al(nbytes + 64), al((reads + 1) * 8), al(reads + 1), al((reads * 2 + 1) * SEQMATCH), al((hits_cap + 1) * HIT),
             256, al(compact_ws_bytes(reads) + 16)]
    return [sum(sizes[:k]) for k in range(8)]


def staged_content(reads, nbytes, hits_cap):
    """What each region has to hold: the span behind a lead of up to 15 bytes, n + 1 offsets, a count and two matches
    per read, hits_cap records, the total, the compaction's workspace behind its own alignment to 16."""
    return [15 + nbytes, (reads + 1) * 8, reads, reads * 2 * SEQMATCH, hits_cap * HIT, 8, compact_ws_bytes(reads) + 15]


def staged_cases():
    return [(r, b, h) for r in READS for b in BYTES for h in sorted({0, 1, r})]


def staged_job(r, b, h):
    return "staged %d %d %d %d" % (r, b, h, compact_ws_bytes(r))


def test_staged_layout(program, tmp_path):
    cases = staged_cases()
    got = run(program, tmp_path, [staged_job(*c) for c in cases])
    for c, g in zip(cases, got):
        assert g == model_staged(*c), c
        assert g[0] == 0 and all(x % 256 == 0 for x in g), c                          # the order is the list's; alignment
        for k, need in enumerate(staged_content(*c)):                                 # disjoint, the last ends in the block
            assert g[k] + need <= g[k + 1], (c, k)


def test_an_arena_holds_every_pack_it_admits(program, tmp_path):
    """A staged arena sized for (max_reads, max_bytes) — a stream slot — holds the layout of every pack with
    n <= max_reads, bytes <= max_bytes, hits_cap = n; and the packed form of a span whenever the packed entry's own
    capacity test (8a31298 line 2566) passes."""
    rng = np.random.default_rng(9)
    for max_reads, max_bytes in ((1, 0), (64, 150 * 64), (65, 17), (8193, 4096 * 8193), (1000, 255)):
        arena = run(program, tmp_path, [staged_job(max_reads, max_bytes, max_reads)])[0]
        room = [arena[k + 1] - arena[k] for k in range(7)]
        packs = {(n, b) for n in READS if n <= max_reads for b in BYTES if b <= max_bytes} | {(max_reads, max_bytes)}
        packs = sorted(packs)
        got = run(program, tmp_path, [staged_job(n, b, n) for n, b in packs])
        for (n, b), g in zip(packs, got):
            assert all(g[k + 1] - g[k] <= room[k] for k in range(7)), (max_reads, max_bytes, n, b)
            assert all(need <= room[k] for k, need in enumerate(staged_content(n, b, n)))
        spans = [(0, 0), (0, max_bytes), (5, 5 + max_bytes), (16, 16 + max_bytes), (31, 31 + max_bytes // 2)]
        spans += [(int(b0), int(b0) + int(rng.integers(0, max_bytes + 1))) for b0 in rng.integers(0, 1 << 40, 20)]
        got = run(program, tmp_path, ["packed %d %d" % s for s in spans])
        fit = 0
        for (b0, b1), (c0, nc, iv_at, nbytes) in zip(spans, got):
            assert (c0, nc) == (b0 >> 4, ((b1 + 15) >> 4) + 4 - (b0 >> 4))                # 8a31298 line 2563
            assert (iv_at, nbytes) == (al(nc * 4, 16), al(nc * 4, 16) + nc * 2)           # lines 2565-2566
            assert 16 * c0 <= b0 and 16 * (c0 + nc) >= b1 + 64                            # the span and four chunks past it
            if nbytes <= max_bytes + 64:                                                  # the entry's capacity test
                fit += 1
                assert nbytes <= room[0]
        assert fit >= 1


# ---- the zero-copy block -------------------------------------------------------------------------------------------
def model_zc(n, nbytes, staged):
    """8a31298 zc_submit, lines 1483-1490: | flag 64 | offsets | matches | counts | bases |, reserve + 64."""
    sz_flag, sz_off, sz_cnt, sz_m = 64, al((n + 1) * 8, 16), al(n, 16), n * 32
    sz_b = al(nbytes + 64, 16) if staged else 0
    return [sz_flag, sz_flag + sz_off, sz_flag + sz_off + sz_m, sz_flag + sz_off + sz_m + sz_cnt,
            sz_flag + sz_off + sz_cnt + sz_m + sz_b + 64]


def test_zero_copy_layout(program, tmp_path):
    cases = [(n, b, s) for n in READS for b in BYTES for s in (0, 1)]
    got = run(program, tmp_path, ["zc %d %d %d" % c for c in cases])
    for (n, b, s), g in zip(cases, got):
        assert g == model_zc(n, b, s), (n, b, s)
        assert all(x % 16 == 0 for x in g)
        content = [(n + 1) * 8, n * 2 * SEQMATCH, n, b if s else 0]
        assert g[0] == 64                                                                 # the completion word's 64 bytes
        for k, need in enumerate(content):
            assert g[k] + need <= g[k + 1], (n, b, s, k)
