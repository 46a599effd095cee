"""libgfdeflate.so past one member per scan thread (include/gf_deflate.h): ``gf_df_deflate_device`` over texts of 65 to
2050 members, held to the host model member by member with the helpers of tests/test_deflate_gpu.py as they are — every
output byte, offset, total and sentinel check they make.  What is new is the input.  ``gf_df_k_scan`` is the one-block
scan ``gf_scan_totals_block`` over the members' sizes (SCAN_THREADS threads, ``per = ceil(members / SCAN_THREADS)``
sizes a thread): the other module stays inside its first wavefront at ``per = 1``; here every member count is named by
what it crosses.  ``gf_df_k_move`` packs the slots with a byte head, funnel-shifted words and a byte tail: the texts are
drawn from a pool of full members whose sizes take every residue mod 4, in a seeded order that meets all 16 combinations
of (destination mod 4, size mod 4).  A true length on the device far below the capacity — the shape
``ReadWriter(deflate="device")`` gives the call — leaves most members absent, and the output of 2050 members is
inflated again on the device, four full windows a workgroup.

The conditions on the inputs are asserted without a GPU, on the host model alone, and the same test holds the constants
to the sources: a later change of a size fails here and does not quietly bring the coverage back to ``per = 1``."""
import functools
import os
import re

import numpy as np
import pytest

from genefuserust_amd import deflate as df
from tests import bgzf_members as bm
from tests import deflate_cases as dc
from tests.test_deflate_gpu import JUNK, against_the_host, device_deflate, host_member, host_members
from tests.test_scan_second_level import SCAN_CSRC, SCAN_THREADS, WAVE, _define, scan_shape

T = dc.TEXT
SLOT = 65536                        # GF_DF_SLOT: a member's slot in the workspace
INFLATE_GROUPS = 512                # the grid of gf_if_k_inflate (tests/test_deflate_gpu.py states it the same way)
TAILS = (1, 4097)                   # bytes of text in the last member

# M: (per, threads that have a run, length of the last run) of gf_df_k_scan
COUNTS = {
    WAVE + 1: (1, WAVE + 1, 1),                                   # the scan block's second wavefront
    SCAN_THREADS: (1, SCAN_THREADS, 1),                           # the last size at per = 1
    SCAN_THREADS + 1: (2, SCAN_THREADS // 2 + 1, 1),              # per = 2, 513 busy threads, a last run of 1
    SCAN_THREADS + SCAN_THREADS // 2 + 1: (2, 769, 1),            # per = 2, 769 busy threads, a last run of 1
    2 * SCAN_THREADS + 2: (3, 684, 1),                            # per = 3, 684 busy threads, a last run of 1
}
LARGEST = 2 * SCAN_THREADS + 2
# the member count of the true-length and inflate cases: the largest, as long as the cases at it take no longer than all
# of tests/test_deflate_gpu.py does (DESIGN.md has the times); otherwise 1537, never less than 1025
TRUE_LEN_M = LARGEST


# (the texts tests/deflate_cases.py had when the seeds of ``order_of`` were chosen)
POOL_TEXTS = ("fastq", "binned", "one_byte_value", "period_2", "period_3", "all_values", "random", "motif_32768",
              "chained_258")


@functools.lru_cache(maxsize=None)
def pool():
    """The first and second member's text of each of the nine texts: 18 full members."""
    return tuple(dc.texts()[name][k * T:(k + 1) * T] for name in POOL_TEXTS for k in (0, 1))


@functools.lru_cache(maxsize=None)
def order_of(M: int):
    """Which pool entry each of the first M - 1 members is.  (The seed is the first that gave every M all 16
    combinations of test_the_pool_and_the_orders_reach_every_head_shift_and_tail: at 64 members a draw can miss one.)"""
    return tuple(int(x) for x in np.random.default_rng(1000 + M).integers(0, len(pool()), M - 1))


@functools.lru_cache(maxsize=None)
def text_of(M: int) -> bytes:
    """M members: M - 1 pool entries in a seeded order, then a tail."""
    p = pool()
    tail = dc.texts()["binned"][:TAILS[M % 2]]
    return b"".join([p[i] for i in order_of(M)] + [tail])


def leads(M: int):
    return dict(lead=M % 16, out_lead=(5 * M) % 16)


# ---- without a GPU: the sizes are the sources', and the inputs reach what they are meant to reach ----------------------

def test_sizes_are_the_sources_defines():
    assert _define("gf_df_core.h", "GF_DF_TEXT") == "%du" % T and T == df.TEXT == 65280
    assert _define("gf_df_kernels.h", "GF_DF_SLOT") == "%du" % SLOT
    assert int(_define("gf_scan_common.h", "GF_SCAN_TOTALS_THREADS")) == SCAN_THREADS == 1024
    launch = open(os.path.join(SCAN_CSRC, "gf_deflate.hip")).read()
    assert len(re.findall(r"hipLaunchKernelGGL\(gf_df_k_scan, dim3\(1\), dim3\(GF_SCAN_TOTALS_THREADS\)", launch)) == 1
    kernels = open(os.path.join(SCAN_CSRC, "gf_df_kernels.h")).read()
    body = re.search(r"__global__[^;{]*?\bvoid gf_df_k_scan\([^)]*\)\s*\{(.*?)\n\}", kernels, flags=re.S)
    assert body and len(re.findall(r"\bgf_scan_totals_block\(sizes, member_off, members\)", body.group(1))) == 1
    # the split into runs is the shared body's alone
    split = r"per = \((?:ntiles|n|members) \+ GF_SCAN_TOTALS_THREADS - 1\) / GF_SCAN_TOTALS_THREADS;"
    assert not re.findall(split, kernels)
    assert len(re.findall(split, open(os.path.join(SCAN_CSRC, "gf_scan_common.h")).read())) == 1


def test_member_counts_cross_the_thresholds():
    assert sorted(COUNTS) == [65, 1024, 1025, 1537, 2050]
    for M, (per, busy, last) in COUNTS.items():
        assert scan_shape(M) == (M, per, busy, last), M
        assert df.members(len(text_of(M))) == M and len(text_of(M)) == (M - 1) * T + TAILS[M % 2]
    assert scan_shape(WAVE)[2] == WAVE and scan_shape(SCAN_THREADS + 1)[1] == 2 and scan_shape(2 * SCAN_THREADS + 1)[1] == 3
    assert {len(text_of(M)) % T for M in COUNTS} == set(TAILS)
    # the true length of the second case lies inside a member in the middle of a thread's run of three
    assert TRUE_LEN_M in COUNTS and TRUE_LEN_M > SCAN_THREADS
    per = scan_shape(TRUE_LEN_M)[1]
    inside = _inside(TRUE_LEN_M)
    assert (per == 3 and inside % per == 1) or (per == 2 and inside % per == 0)
    assert TRUE_LEN_M // 2 < inside < TRUE_LEN_M - TRUE_LEN_M // 4
    # the inflate's grid-stride loop takes several full windows one after the other in one workgroup
    assert TRUE_LEN_M // INFLATE_GROUPS >= 3


def test_the_pool_and_the_orders_reach_every_head_shift_and_tail():
    """On the host model alone: the pool's member sizes take all four residues mod 4 and both kinds, and for every M
    the seeded sequence meets all 16 combinations of (where the member lands mod 4, its size mod 4) — every head, shift
    and tail ``gf_df_k_move`` has.  The output's first byte lies ``out_lead`` behind a 16-byte boundary."""
    members = [host_member(t) for t in pool()]
    assert len(members) == 18 and all(len(t) == T for t in pool())
    sizes = [len(m) for m in members]
    kinds = {bm.block_kinds(m[18:-8])[0] for m in members}
    assert {s % 4 for s in sizes} == {0, 1, 2, 3} and kinds == {0, 2}
    assert len(set(sizes)) >= 8 and min(sizes) < 1024 and max(sizes) == T + df.STORED_OVER
    for M in COUNTS:
        seq = [sizes[i] for i in order_of(M)]
        at = leads(M)["out_lead"] + np.concatenate([[0], np.cumsum(seq)[:-1]])
        met = {(int(a) % 4, s % 4) for a, s in zip(at, seq)}
        assert len(met) == 16, (M, sorted(met))
        assert len(set(order_of(M))) == len(pool()) or M < 100


# ---- on the device -------------------------------------------------------------------------------------------------

def _inside(M: int) -> int:
    """The member the true length of the second case ends in: two thirds into the text."""
    return 2 * M // 3 if scan_shape(M)[1] == 3 else 2 * (M // 3)


@pytest.mark.gpu
@pytest.mark.parametrize("M", sorted(COUNTS))
def test_every_member_count_whole(gpu_device, M):
    got = against_the_host(text_of(M), **leads(M))
    assert len(got) == sum(len(m) for m in host_members(text_of(M)))


@pytest.mark.gpu
def test_true_length_inside_a_member_in_the_middle_of_a_run(gpu_device):
    """A third of the members are absent, and the last live one is the second of its thread's three."""
    M = TRUE_LEN_M
    k = _inside(M)
    true_len = k * T + 12345
    assert df.members(true_len) == k + 1
    against_the_host(text_of(M), true_len, **leads(M))


@pytest.mark.gpu
def test_the_writers_shape_three_members_of_a_capacity_of_thousands(gpu_device):
    """What ``ReadWriter(deflate="device")`` hands the call: the worst-case size as the capacity, the true length on
    the device — here three members in front of M - 3 absent ones."""
    M = TRUE_LEN_M
    got = against_the_host(text_of(M), 2 * T + 1, **leads(M))
    assert got == b"".join(host_members(text_of(M)[:2 * T + 1]))


@pytest.mark.gpu
def test_true_length_zero_at_two_members_a_thread(gpu_device):
    M = SCAN_THREADS + 1
    text = text_of(M)
    assert against_the_host(text, 0, **leads(M)) == b""
    got, off, totals = device_deflate(text, 0, **leads(M))
    assert got == b"" and off == [0] * (M + 1) and totals == [0] * 5       # no member, every offset 0, totals untouched


@pytest.mark.gpu
def test_the_device_inflate_reads_full_windows_one_after_the_other(gpu_device):
    """The output of TRUE_LEN_M members through ``gf_if_walk_blocks`` and ``gf_if_inflate_device``: every status 0 and
    the text is back; a workgroup of the inflate takes four full windows, one after the other."""
    import torch
    from genefuserust_amd import bgzf
    M = TRUE_LEN_M
    text = text_of(M)
    d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    out, member_off, totals = df.deflate_device(d_text)
    t = totals.cpu().tolist()
    want = host_members(text)
    assert t[:3] == [M, len(text), sum(len(m) for m in want)] and t[2] == int(member_off[-1])
    comp = out[:t[2]].cpu().numpy()
    assert comp.tobytes() == b"".join(want)
    walk = bgzf.walk_blocks(comp)
    assert (walk.members, walk.comp_bytes, walk.text_bytes, walk.why) == (M, t[2], len(text), bm.WALK_END)
    assert walk.table[:, 0].tolist() == [int(x) + 18 for x in member_off[:M].cpu().tolist()]
    back = torch.full((len(text) + 16,), JUNK, dtype=torch.uint8, device="cuda")
    status, totals = bgzf.inflate_device(out[:t[2]], torch.from_numpy(walk.table.copy()).cuda(), back)
    assert not status.cpu().numpy().any() and status.numel() == M
    assert totals.cpu().tolist() == [M, -1, 0, len(text)]
    assert torch.equal(back[:len(text)], d_text) and set(back[len(text):].cpu().tolist()) == {JUNK}
