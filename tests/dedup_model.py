"""The predicate of include/gf_dedup.h in plain Python: keys, survivors by the lowest index over a sequence of calls,
the totals and the histogram.  What libgfdedup.so is held to, on the host (tests/test_dedup_core.py) and on the device
(tests/test_dedup_gpu.py).  Nothing here looks at the library's code."""
from collections import namedtuple

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
LEVELS, TOTALS, MIN_SLOTS = 32, 6, 1024
NO_INDEX = (1 << 63) - 1


def mix(x: int) -> int:
    x &= M64
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    x ^= x >> 31
    return x


def H(b: bytes) -> int:
    L = len(b)
    total = 0
    for j in range((L + 7) // 8):
        word = bytes(c & 0xDF for c in b[8 * j:8 * j + 8]).ljust(8, b"\0")
        total += mix(int.from_bytes(word, "little") + (j + 1) * GOLDEN)
    return mix(L + total)


def key(r1: bytes, r2: bytes = None) -> int:
    """K of a single-end read, or of a pair; 0 for a record with no bases."""
    if r2 is None:
        k = H(r1) if r1 else 0
        return (k or 1) if r1 else 0
    if not r1 and not r2:
        return 0
    return mix(H(r1) + mix(H(r2) + 1)) or 1


def home(k: int, slots: int) -> int:
    return k & (slots - 1)


def level(c: int) -> int:
    return min(c, LEVELS - 1)


Offered = namedtuple("Offered", "dup totals")


class Table:
    """The set of (key, first, count) a table holds, whatever its layout, and what each call does to it.  ``slots``: how
    many keys the table has room for; None (the default): room for every key.  A key that is not in a table without room
    is not placed: its record gets no slot, the call counts it in totals [5], and the table stays as it is."""

    def __init__(self, slots: int = None):
        self.first, self.count = {}, {}
        self.offered = 0
        self.slots = slots

    def insert(self, keys, first_index: int = None):
        """One ``gf_dd_insert_device`` call: the totals [0], [1], [2] and [5] it adds."""
        first_index = self.offered if first_index is None else first_index
        new = failed = 0
        for i, k in enumerate(keys):
            if not k:
                continue
            if k not in self.first:
                if self.slots is not None and len(self.first) >= self.slots:
                    failed += 1
                    continue
                new += 1
                self.first[k], self.count[k] = NO_INDEX, 0
            self.first[k] = min(self.first[k], first_index + i)
            self.count[k] += 1
        self.offered = max(self.offered, first_index + len(keys))
        return [len(keys), sum(1 for k in keys if k), new, 0, 0, failed]

    def duplicates(self, keys, first_index: int):
        """One ``gf_dd_remove_device`` call behind the insert of the same keys: 1 for every duplicate; a record whose key
        found no room has no slot and is none."""
        return [int(bool(k) and k in self.first and self.first[k] != first_index + i) for i, k in enumerate(keys)]

    def offer(self, records, first_index: int = None) -> Offered:
        """Insert, then remove: ``records`` are reads (bytes) or pairs of them.  (duplicate flags, the six totals)."""
        first_index = self.offered if first_index is None else first_index
        keys = [key(*r) if isinstance(r, tuple) else key(r) for r in records]
        totals = self.insert(keys, first_index)
        dup = self.duplicates(keys, first_index)
        totals[3] = sum(dup)
        totals[4] = sum(len(b"".join(r) if isinstance(r, tuple) else r) for r, d in zip(records, dup) if d)
        return Offered(dup, totals)

    def entries(self, counted: bool = True):
        return {(k, f, self.count[k]) if counted else (k, f) for k, f in self.first.items()}

    def histogram(self):
        h = [0] * LEVELS
        for c in self.count.values():
            if c:
                h[level(c)] += 1
        return h

