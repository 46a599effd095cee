"""The records that the read QC's tests share (tests/test_read_qc_core.py on the host, tests/test_read_qc_gpu.py on the
device): reads at every edge of the table of include/gf_read_qc.h, short ones for every wavefront of a launch, and the
pairs of the insert histogram.  Built once and left unchanged; the model's answers are computed once too."""
import functools
from typing import List, Tuple

import numpy as np

from tests.adapter_trim_cases import bases_of, pair_cases, rc
from tests.read_qc_model import insert_entry

# the first and the last lane of a round, the last cycle with a row of its own, the tail row, many rounds of it
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 150, 511, 512, 513, 600, 4096, 5000]
BASE_BYTES = np.frombuffer(b"ACGTacgtN." + bytes([0, 255]), dtype=np.uint8)
# below, at and above phred 0, 20 and 30, and the largest
QUAL_BYTES = np.array([32, 33, 52, 53, 62, 63, 126, 255], dtype=np.uint8)
Read = Tuple[bytes, bytes]


def read_of(rng, n: int) -> Read:
    return rng.choice(BASE_BYTES, n).tobytes(), rng.choice(QUAL_BYTES, n).tobytes()


@functools.lru_cache(maxsize=None)
def edge_reads(seed: int = 1) -> Tuple[Read, ...]:
    """Two reads of every length of ``LENGTHS``, in an order that mixes them."""
    rng = np.random.default_rng(seed)
    reads = [read_of(rng, n) for n in LENGTHS + LENGTHS[::-1]]
    return tuple(reads[k] for k in rng.permutation(len(reads)))


@functools.lru_cache(maxsize=None)
def short_reads(n: int, seed: int = 2) -> Tuple[Read, ...]:
    """n reads of 1 to 40 bases."""
    rng = np.random.default_rng(seed)
    return tuple(read_of(rng, int(L)) for L in rng.integers(1, 41, n))


def fragment_pair(rng, insert: int, L1: int, L2: int) -> Tuple[bytes, bytes]:
    """The mates of a fragment of ``insert`` bases; behind a fragment shorter than a mate, random bases."""
    f = bases_of(rng, insert)
    return (f + bases_of(rng, L1))[:L1], (rc(f) + bases_of(rng, L2))[:L2]


@functools.lru_cache(maxsize=None)
def top_pairs() -> Tuple[Tuple[bytes, bytes], ...]:
    """Up to the top of the histogram: two 512-base mates at the last candidate, 994, and at 900; and a pair at the
    first, 30."""
    rng = np.random.default_rng(5)
    return fragment_pair(rng, 994, 512, 512), fragment_pair(rng, 900, 512, 512), fragment_pair(rng, 30, 100, 100)


@functools.lru_cache(maxsize=None)
def insert_pairs() -> Tuple[Tuple[bytes, bytes], ...]:
    return tuple(pair_cases("illumina")) + top_pairs()


@functools.lru_cache(maxsize=None)
def insert_entries() -> Tuple[int, ...]:
    """The model's entry of every pair of ``insert_pairs()``, computed once."""
    return tuple(insert_entry(a, b) for a, b in insert_pairs())


def with_quals(reads: List[bytes], q: int = 70) -> List[Read]:
    return [(b, bytes([q]) * len(b)) for b in reads]
