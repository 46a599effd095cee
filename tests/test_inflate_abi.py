"""gf_if_inflate_device (include/gf_inflate.h) on the MI355X against zlib, member by member: every block kind, the
members zlib cannot emit and the malformed ones — inputs the host build of the same decoder has passed
(tests/test_inflate_core.py) — at odd offsets, with sentinels around the output."""
import gzip

import numpy as np
import pytest

from tests import bgzf_members as bm

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def good():
    """[(name, text, member)]: every good kind, once."""
    cases = bm.kinds() + [("period_%d" % p, bm.periodic(p), bm.member(bm.periodic(p))) for p in bm.PERIODS]
    full = bm.fastq_text(65536, seed=4)
    cases.append(("isize_65536", full, bm.member(full)))
    cases += bm.hand_assembled() + bm.valid_dynamic()
    for name, text, m in cases:
        assert gzip.decompress(m) == text, name
    return cases


def inflate(comp: bytes, table: np.ndarray, out_cap: int):
    """(output bytes, statuses, totals) of one call over a sentinel-filled output."""
    import torch
    from genefuserust_amd import bgzf
    dev = torch.device("cuda", 0)
    d_comp = torch.from_numpy(np.frombuffer(comp, dtype=np.uint8).copy()).to(dev)
    d_table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int64)).to(dev)
    out = torch.full((out_cap,), SENTINEL, dtype=torch.uint8, device=dev)
    status, totals = bgzf.inflate_device(d_comp, d_table, out)
    return out.cpu().numpy().tobytes(), status.cpu().numpy(), totals.cpu().numpy().tolist()


def check(cases, want=None, text_gap=3, comp_gap=1, text_base=5):
    """``cases`` [(name, text, member)] in one call; ``want``: the statuses (default: all good)."""
    want = [0] * len(cases) if want is None else want
    comp, table, need = bm.table_of([m for _, _, m in cases], text_gap=text_gap, comp_gap=comp_gap, text_base=text_base)
    out, status, totals = inflate(comp, table, need + 7)
    assert status.tolist() == want, [(c[0], int(s), w) for c, s, w in zip(cases, status, want) if s != w]
    expect = bytearray([SENTINEL]) * (need + 7)
    for (name, text, _), row, w in zip(cases, table, want):
        if w == 0:
            expect[row[2]:row[2] + row[3]] = text
            assert out[row[2]:row[2] + row[3]] == text, name
    assert out == bytes(expect)      # sentinels between the texts, and in the failed members' own ranges
    bad = [k for k, w in enumerate(want) if w]
    assert totals == [len(want) - len(bad), bad[0] if bad else -1, want[bad[0]] if bad else 0,
                      sum(len(c[1]) for c, w in zip(cases, want) if w == 0)]


def test_every_kind_against_zlib(gpu_device, good):
    check(good)
    # every output alignment modulo 16 for the first member, texts back to back
    for base in range(16):
        check(good[:5], text_gap=0, comp_gap=0, text_base=base)


def test_codes_at_their_limits(gpu_device):
    """``deep_codes`` (the host build has passed them in tests/test_inflate_core.py): codes of 13 to 15 bits, a
    code-length code of 5 to 7 bits, the largest repeats, length 258 both ways and distance 32768, by hand, by this
    project's encoder and by zlib: every text back, status 0, at odd offsets between sentinels."""
    cases = bm.deep_codes()
    for name, text, m in cases:
        assert gzip.decompress(m) == text, name
    check(cases)
    hand = [c for c in cases if not c[0].endswith("_own") and "_zlib_" not in c[0]]
    assert len(hand) == 3
    for base in (0, 1, 7, 15):
        check(hand + cases[:2], text_gap=0, comp_gap=0, text_base=base)


@pytest.mark.parametrize("count", [1, 2, 513])
def test_member_counts(gpu_device, good, count):
    """One, two, one more than the grid holds (the members stride)."""
    small = [c for c in good if len(c[1]) <= 20000 or c[0] in ("level6", "all_a")]
    check([small[k % len(small)] for k in range(count)])


def test_1025_one_byte_members(gpu_device):
    texts = [bytes([65 + k % 26]) for k in range(1025)]
    check([("byte_%d" % k, t, bm.member(t)) for k, t in enumerate(texts)], text_gap=0, comp_gap=0, text_base=1)


def test_malformed_members_among_good_ones(gpu_device, good):
    bad = bm.malformed()
    fillers = [c for c in good if c[0] in ("level6", "one_byte", "empty", "period_3", "len3_dist1", "fixed")]
    cases, want = [], []
    for k, (name, m, status) in enumerate(bad):
        cases += [(name, b"", m), fillers[k % len(fillers)]]
        want += [status, 0]
    check(cases, want)
    check(cases[1:], want[1:])       # the first failed member is not the first member


def test_rows_that_point_outside_are_statuses(gpu_device):
    text = bm.fastq_text(1000, seed=2)
    comp, table, need = bm.table_of([bm.member(text)] * 8)
    table[1, 0] = len(comp) - 3
    table[2, 0] = -1
    table[3, 2] = need - 999
    table[4, 2] = -1
    table[5, 3] = bm.MAX_TEXT + 1
    table[6, 1] = bm.MAX_TEXT + 1
    out, status, totals = inflate(comp, table, need)
    assert status.tolist() == [0] + [bm.BAD_ROW] * 6 + [0]
    assert out[:1000] == text and out[7000:8000] == text and set(out[1000:7000]) == {SENTINEL}
    assert totals == [2, 1, bm.BAD_ROW, 2000]


def test_no_members(gpu_device):
    import torch
    from genefuserust_amd import bgzf
    dev = torch.device("cuda", 0)
    empty = torch.empty(0, dtype=torch.uint8, device=dev)
    status, totals = bgzf.inflate_device(empty, torch.empty((0, 6), dtype=torch.int64, device=dev), empty)
    assert status.numel() == 0 and totals.cpu().tolist() == [0, -1, 0, 0]
