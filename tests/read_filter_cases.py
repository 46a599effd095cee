"""The reads that the read filter's tests share (tests/test_read_filter_core.py on the host, tests/test_read_filter_gpu.py
on the device): for given settings, reads at every edge of the predicate, and random ones.  Built once per settings
and left unchanged."""
from typing import List, Tuple

import numpy as np

from tests.read_filter_model import Settings

LENGTHS = [0, 1, 3, 4, 14, 15, 16, 63, 64, 65, 127, 128, 129, 150, 255, 256, 257, 4095, 4096, 4097]
GOOD, BAD = 33 + 40, 33 + 2        # 'I' and '#'
Read = Tuple[bytes, bytes]

# the settings the kernel is held to the model on: the defaults, the tail cut at windows 1, 4 and 64, each single switch
# off (0) in turn, and the largest values the library takes
SETTINGS = {
    "defaults": Settings(),
    "window 4": Settings(cut_tail_window=4),
    "window 1": Settings(cut_tail_window=1, cut_tail_mean=30),
    "window 64": Settings(cut_tail_window=64, cut_tail_mean=25),
    "no poly-G": Settings(poly_g_min=0, cut_tail_window=5),
    "mean 0": Settings(cut_tail_window=4, cut_tail_mean=0),
    "any length": Settings(length_required=0, cut_tail_window=4),
    "no N": Settings(n_base_limit=0),
    "phred 0": Settings(qualified_phred=0),
    "percent 0": Settings(unqualified_percent=0),
    "largest": Settings(poly_g_min=4096, cut_tail_window=64, cut_tail_mean=93, length_required=4096, n_base_limit=1 << 30,
                        qualified_phred=93, unqualified_percent=100),
}


def bases_of(rng, n: int, last_not_g: bool = True) -> bytes:
    b = bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tobytes())
    if n and last_not_g and b[-1] in b"Gg":
        b[-1] = ord("A")
    return bytes(b)


def edge_reads(s: Settings, seed: int = 1) -> List[Read]:
    rng = np.random.default_rng(seed)
    good = lambda n: bytes([GOOD]) * n   # noqa: E731
    out: List[Read] = []
    # every length: a clean read, and one with anything for qualities
    for L in LENGTHS:
        out.append((bases_of(rng, L), good(L)))
        out.append((bases_of(rng, L, False), rng.integers(33, 75, L, dtype=np.uint8).tobytes()))
    # poly-G tails: one short of the least, the least, the whole read; both cases; a run broken one base from the end
    g = max(s.poly_g_min, 2)
    for L in (g + 20, 64, 150, 257, 4096):
        if L < g + 2:
            continue
        for run in (g - 1, g, g + 1):
            tail = bytes(rng.choice(np.frombuffer(b"Gg", dtype=np.uint8), run).tobytes())
            out.append((bases_of(rng, L - run) + tail, good(L)))
        out.append((b"G" * L, good(L)))
        out.append((b"g" * (L // 2) + b"G" * (L - L // 2), good(L)))
        out.append((bases_of(rng, L - g - 2) + b"G" * g + b"AG", good(L)))
        out.append((bases_of(rng, L - g - 2) + b"G" * g + b"Ng", good(L)))
    out.append((b"G" * (g - 1), good(g - 1)))
    # the tail cut: window sums one short of W M and at it; the window at e = W, at e = e1, nowhere; e1 < W
    W, M = max(s.cut_tail_window, 1), s.cut_tail_mean
    at = bytes([33 + M]) * W
    short = at[:-1] + bytes([33 + max(M - 1, 0)])
    for L in (W, W + 1, W + 16, 2 * W + 37, 150, 300, 4096):
        if L < W:
            continue
        bad = lambda n: bytes([BAD if M > 2 else 33]) * n   # noqa: E731
        for win in (at, short):
            out.append((bases_of(rng, L), win + bad(L - W)))                      # e = W
            out.append((bases_of(rng, L), bad(L - W) + win))                      # e = L
            mid = (L - W) // 2
            out.append((bases_of(rng, L), bad(mid) + win + bad(L - W - mid)))
        out.append((bases_of(rng, L), bad(L)))                                    # nowhere
        if L > g + W:                                                             # e = e1 below a poly-G tail
            out.append((bases_of(rng, L - g) + b"G" * g, bad(L - W - g) + at + good(g)))
    for L in (1, W - 1, W // 2):
        if 0 < L < W:
            out.append((bases_of(rng, L), good(L)))
    # N: the limit and one more; lower case is no N; bytes outside the alphabet are
    k = min(s.n_base_limit, 4000)
    for L in (max(k + 20, 40), 150, 4096):
        for n_count in (k, k + 1):
            if n_count > L - 1:
                continue
            b = bytearray(bases_of(rng, L))
            for i, p in enumerate(rng.choice(L - 1, n_count, replace=False).tolist()):
                b[p] = b"N.n\x00\xffX-*@[`{"[i % 12]
            out.append((bytes(b), good(L)))
        out.append((bases_of(rng, L).lower(), good(L)))
    out.append((b"ACGTacgtNn" * 10 + b"A", good(101)))
    # the low share: exactly the percentage, and one base over
    for L in (100, 20, 200, 4000):
        low = s.unqualified_percent * L // 100
        for n_low in (low, low + 1):
            if n_low > L:
                continue
            q = bytearray(good(L))
            below = 33 + max(s.qualified_phred - 1, 0)
            for p in rng.choice(L, n_low, replace=False).tolist():
                q[p] = below
            out.append((bases_of(rng, L), bytes(q)))
        out.append((bases_of(rng, L), bytes([33 + s.qualified_phred]) * L))       # at the threshold: not low
    # quality bytes below 33, at 126 and past it
    for L in (40, 150):
        for vals in ([0, 10, 32, 33], [126], [126, 33], [127, 128, 200, 255], [32, 126]):
            out.append((bases_of(rng, L), bytes(rng.choice(np.array(vals, dtype=np.uint8), L).tobytes())))
    return out


def random_reads(n: int, seed: int, longest: int = 300) -> List[Read]:
    """Reads of 0 .. ``longest`` bases: G tails, N runs, lower case, tails of falling quality, junk bytes."""
    rng = np.random.default_rng(seed)
    out: List[Read] = []
    for _ in range(n):
        L = int(rng.integers(0, longest + 1))
        b = bytearray(bases_of(rng, L, False))
        q = bytearray(rng.integers(33 + 20, 33 + 42, L, dtype=np.uint8).tobytes())
        kind = int(rng.integers(0, 8))
        if L:
            if kind == 0:
                t = int(rng.integers(0, min(L, 30) + 1))
                b[L - t:] = rng.choice(np.frombuffer(b"Gg", dtype=np.uint8), t).tobytes()
            elif kind == 1:
                for p in rng.integers(0, L, int(rng.integers(0, 12))).tolist():
                    b[p] = ord("N")
            elif kind == 2:
                t = int(rng.integers(0, L + 1))
                q[L - t:] = rng.integers(33, 33 + 25, t, dtype=np.uint8).tobytes()
            elif kind == 3:
                q = bytearray(rng.integers(33, 33 + 30, L, dtype=np.uint8).tobytes())
            elif kind == 4:
                b = bytearray(bytes(b).lower())
                q = bytearray(rng.integers(0, 256, L, dtype=np.uint8).tobytes())
            elif kind == 5:
                b = bytearray(rng.integers(0, 256, L, dtype=np.uint8).tobytes())
        out.append((bytes(b), bytes(q)))
    return out
