"""Junction reads that sit next to map_read's gates (indexer.rs:353-360 the vote gate, :440-449 the
mask gate, :616-679 run_end's tolerance and the span gate): deterministic, numpy only, no GPU, no file.

Every read joins two gene parts (three in one tie family), each part on either strand, on the same
or on different genes; half of the reads are reverse-complemented as a whole.  Lengths are 100, 150,
251 and 300 before the edits and 98..302 after them.  The families differ in the edits:

  clusters     1-7 substitution clusters; a cluster substitutes its first and its last base, so a
               cluster of width w <= 17 leaves exactly w bases that no matching window covers
  minor        the shorter part is 30-55 bases long and holds 0-2 substitutions
  major        the break lies within 8 bases of the middle; length 100 unedited or with clusters,
               longer reads with clusters
  inner9/10/11 exactly one cluster of that width, at least 25 bases inside a part of 70 bases or
               more, nothing else: the run stays whole / is split / the mask gate rejects the read
  interleaved  300 bases of alternating pieces of A and B, 20-23 bases wide, each piece on its own
               part's diagonal: best runs of 19-22 bases, results with no, one and two segments
  indel1       one or two 1-bp indels (the +-1 diagonal neighbours), at least 5 bases inside
  indel2       one or two indels of which one is 2 bp wide
  n_lower      1-5 bases set to N or lower-cased
  tie2         both parts equally long, unedited, in both orders and all four strand combinations
  tie3         three parts, the second and third equally long

One family is no junction.  A junction read can never make the proof of the first-place gate tight: the
other part's windows all count as able to vote.  Only where a window votes for two diagonals at once can
a read pass both gates with no more than 20 voting windows in all:

  dupe         50-66 bases from inside a stretch of the genes that occurs two to five times, unedited or
               with one substitution: every window votes for each copy's diagonal, first and second place
               tie at the number of voting windows, 15-26, and the first diagonal takes the whole read
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from tests.helpers import rc

LENGTHS = (100, 150, 251, 300)
CLUSTER_WIDTHS = (1, 1, 1, 2, 3, 5, 9, 10, 11, 12)
_OTHER = {ord("A"): b"CGT", ord("C"): b"GTA", ord("G"): b"TAC", ord("T"): b"ACG"}


def _part(rng, genes: Sequence[bytes], n: int) -> bytes:
    """n bases of a random gene at a random place, on either strand."""
    while True:
        g = genes[int(rng.integers(0, len(genes)))]
        if len(g) > n + 2:
            break
    p = int(rng.integers(1, len(g) - n))
    s = g[p:p + n].upper()
    return rc(s) if rng.random() < 0.5 else s


def _junction(rng, genes, L: int, brk: int) -> bytearray:
    return bytearray(_part(rng, genes, brk) + _part(rng, genes, L - brk))


def _substitute(rng, read: bytearray, pos: int) -> None:
    read[pos] = _OTHER.get(read[pos], b"ACG")[int(rng.integers(0, 3))]


def _cluster(rng, read: bytearray, pos: int, w: int) -> None:
    _substitute(rng, read, pos)
    if w > 1:
        _substitute(rng, read, pos + w - 1)


def _clusters(rng, read: bytearray, n: int) -> None:
    for _ in range(n):
        w = int(rng.choice(CLUSTER_WIDTHS))
        _cluster(rng, read, int(rng.integers(0, len(read) - w + 1)), w)


def _interleaved(rng, genes) -> bytearray:
    """Alternating pieces of A and B: a piece at read position pos is A[pos:pos+w], so every piece
    of a part votes for that part's one diagonal.  Each part has a widest piece of its own, and most
    of its pieces are that wide, so that the best run's span is known and the votes stay near 20."""
    L = 300
    a, b = _part(rng, genes, L), _part(rng, genes, L)
    cap = (int(rng.integers(20, 24)), int(rng.integers(20, 24)))
    out, pos, side = bytearray(), 0, int(rng.integers(0, 2))
    while pos < L:
        w = cap[side] if rng.random() < 0.7 else int(rng.integers(20, cap[side] + 1))
        out += (a, b)[side][pos:pos + w]
        pos += w
        side ^= 1
    return out[:L]


def _dupe_stretches(genes: Sequence[bytes], min_windows: int = 60) -> List[Tuple[int, int, int]]:
    """(gene, first base, windows) of every run of at least `min_windows` consecutive 16-base windows whose
    k-mer occurs two to five times on the genes' forward strands."""
    code = np.full(256, 4, dtype=np.uint64)
    for k, ch in enumerate(b"ACGT"):
        code[ch] = k
    keys = []
    for g in genes:
        c = code[np.frombuffer(g.upper(), dtype=np.uint8)]
        n = c.size - 15
        key, bad = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=bool)
        for j in range(16):
            key = (key << np.uint64(2)) | (c[j:j + n] & np.uint64(3))
            bad |= c[j:j + n] == 4
        key[bad] = np.uint64(1 << 40) + np.arange(int(bad.sum()), dtype=np.uint64)   # (unique: never a repeat)
        keys.append(key)
    _, inverse, counts = np.unique(np.concatenate(keys), return_inverse=True, return_counts=True)
    fold = counts[inverse]
    runs, base = [], 0
    for gi, key in enumerate(keys):
        ok = np.concatenate(([False], (fold[base:base + key.size] >= 2) & (fold[base:base + key.size] <= 5), [False]))
        edges = np.flatnonzero(ok[1:] != ok[:-1])
        runs += [(gi, int(a), int(b - a)) for a, b in zip(edges[0::2], edges[1::2]) if b - a >= min_windows]
        base += key.size
    return runs


_INDELS = ((-1, "del1"), (1, "ins1"), (-2, "del2"), (2, "ins2"))


def _indels(rng, read: bytearray, kinds) -> bytearray:
    for k in kinds:
        d = _INDELS[k][0]
        p = int(rng.integers(5, len(read) - 5 - abs(d)))
        if d < 0:
            del read[p:p - d]
        else:
            read[p:p] = bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, size=d))
    return read


def gate_reads(genes: Sequence[bytes], seed: int, n: int = 4000) -> List[Tuple[str, bytes]]:
    """About n (family, read) pairs drawn from `genes` (raw gene slices); the same for the same arguments."""
    rng = np.random.default_rng(seed)
    genes = [g for g in genes if g is not None and len(g) >= 640]
    out: List[Tuple[str, bytes]] = []
    unit = n / 4000.0

    def emit(family: str, read) -> None:
        read = bytes(read)
        out.append((family, rc(read) if rng.random() < 0.5 else read))

    def length() -> int:
        return int(rng.choice(LENGTHS))

    for _ in range(int(800 * unit)):
        L = length()
        read = _junction(rng, genes, L, int(rng.integers(30, L - 29)))
        _clusters(rng, read, int(rng.integers(1, 8)))
        emit("clusters", read)

    for _ in range(int(600 * unit)):
        L, m = length(), int(rng.integers(30, 56))
        left = rng.random() < 0.5
        read = _junction(rng, genes, L, m if left else L - m)
        lo = 0 if left else L - m
        for _ in range(int(rng.integers(0, 3))):
            _substitute(rng, read, lo + int(rng.integers(0, m)))
        emit("minor", read)

    for k in range(int(700 * unit)):
        L = 100 if k % 2 == 0 else int(rng.choice(LENGTHS[1:]))
        read = _junction(rng, genes, L, L // 2 + int(rng.integers(-8, 9)))
        if L > 100:
            _clusters(rng, read, int(rng.integers(2, 8)))
        elif k % 4 == 0:
            _clusters(rng, read, int(rng.integers(1, 3)))
        emit("major", read)

    for k in range(int(300 * unit)):
        L, w = int(rng.choice(LENGTHS[1:])), 9 + k % 3
        big = int(rng.integers(70, L - 39))          # the part that takes the cluster; the other keeps >= 40
        first = rng.random() < 0.5
        read = _junction(rng, genes, L, big if first else L - big)
        p = int(rng.integers(25, big - 25 - w + 1)) + (0 if first else L - big)
        _cluster(rng, read, p, w)
        emit("inner%d" % w, read)

    for _ in range(int(500 * unit)):
        emit("interleaved", _interleaved(rng, genes))

    for k in range(int(500 * unit)):
        L = length()
        read = _junction(rng, genes, L, int(rng.integers(30, L - 29)))
        if k % 2 == 0:
            kinds = [int(x) for x in rng.permutation(2)[:int(rng.integers(1, 3))]]
        else:   # one 2-bp indel, alone or with a 1-bp one of the other direction (the length stays within 2)
            two = int(rng.integers(2, 4))
            kinds = [two] + ([3 - two] if rng.random() < 0.5 else [])
        emit("indel1" if k % 2 == 0 else "indel2", _indels(rng, read, kinds))

    for _ in range(int(250 * unit)):
        L = length()
        read = _junction(rng, genes, L, int(rng.integers(30, L - 29)))
        for p in rng.integers(0, L, size=int(rng.integers(1, 6))):
            read[p] = ord("N") if rng.random() < 0.5 else ord(chr(read[p]).lower())
        emit("n_lower", read)

    for k in range(int(24 * unit)):
        L = (150, 300, 100)[k % 3]
        g = [_part(rng, genes, L // 2), _part(rng, genes, L // 2)]
        for a, b in ((0, 1), (1, 0)):
            for ra in (False, True):
                for rb in (False, True):
                    emit("tie2", (rc(g[a]) if ra else g[a]) + (rc(g[b]) if rb else g[b]))

    for _ in range(int(150 * unit)):
        L = int(rng.choice(LENGTHS[1:]))
        m = int(rng.integers(36, min(L // 3, 60) + 1))
        emit("tie3", _part(rng, genes, L - 2 * m) + _part(rng, genes, m) + _part(rng, genes, m))

    stretches = _dupe_stretches(genes)
    for k in range(int(300 * unit) if stretches else 0):
        gi, a, nw = stretches[int(rng.integers(0, len(stretches)))]
        L = int(rng.integers(50, min(66, nw + 15) + 1))
        p = a + int(rng.integers(0, nw + 15 - L + 1))
        read = bytearray(genes[gi][p:p + L].upper())
        if rng.random() < 0.5:
            read = bytearray(rc(bytes(read)))
        if k % 2:
            _substitute(rng, read, int(rng.choice([0, 1, 2, 3, L - 4, L - 3, L - 2, L - 1])))
        emit("dupe", read)

    return out
