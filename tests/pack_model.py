"""The block of include/gf_scan_pack.h stated in numpy, for tests/test_scan_pack_abi.py (no GPU) and
tests/test_scan_pack.py (against gf_pk_pack_device, byte for byte).  Nothing here looks at the library or its
sources."""
from typing import NamedTuple, Optional, Sequence

import numpy as np

OVER_RETRY, OVER_HITS, OVER_NAMES, BAD_SCAN = 1, 2, 4, 8
SECTIONS = ("records", "bases", "quals", "offsets", "names")


class ModelScan(NamedTuple):
    """One scan and its names as they lie in memory: the arrays' sizes are the capacities (``hits`` uint8[cap, 64],
    ``bases`` / ``quals`` / ``names`` uint8, ``totals`` int64[8], ``name_off`` int64[cap + 1], ``name_totals``
    int64[4])."""
    hits: np.ndarray
    bases: np.ndarray
    quals: np.ndarray
    totals: np.ndarray
    names: np.ndarray
    name_off: np.ndarray
    name_totals: np.ndarray


def make_scan(rng, records: int, read_bytes: int, name_bytes: int, spare=(3, 40, 29), over: int = 0,
              names_over: bool = False, merged: int = 5, retried: int = 7, missing: int = 0) -> ModelScan:
    """A scan with ``records`` records, ``read_bytes`` bytes of reads and ``name_bytes`` of names, random bytes all of
    them, and ``spare`` = (rows, read bytes, name bytes) of capacity behind the counts filled with non-zero garbage;
    garbage offsets behind the last one too.  ``over``: the scan's own overflow bits — its totals then say more than
    its capacities, as a real scan's do with bit 2; ``names_over``: the names' bit, with a total beyond names_cap."""
    def garbage(n):
        return rng.integers(1, 256, size=n, dtype=np.uint8)
    hits_cap, bytes_cap, names_cap = records + spare[0], read_bytes + spare[1], name_bytes + spare[2]
    hits = garbage(hits_cap * 64).reshape(hits_cap, 64)
    cuts = np.sort(rng.integers(0, name_bytes + 1, size=max(records - 1, 0))) if records else np.empty(0, dtype=np.int64)
    off = rng.integers(1 << 40, 1 << 41, size=hits_cap + 1, dtype=np.int64)
    off[:records + 1] = np.concatenate(([0], cuts, [name_bytes]))[:records + 1] if records else [0]
    if records == 0:
        assert name_bytes == 0
    totals = np.array([records, read_bytes, merged, retried, over, 0, 0, 0], dtype=np.int64)
    if over & OVER_HITS:
        totals[0], totals[1] = hits_cap + 9, bytes_cap + 100
    name_totals = np.array([records, name_bytes, 0, missing], dtype=np.int64)
    if names_over:
        name_totals[1:3] = names_cap + 11, 1
    return ModelScan(hits, garbage(bytes_cap), garbage(bytes_cap), totals, garbage(names_cap), off, name_totals)


def _clamp(v, cap):
    return max(0, min(int(v), int(cap)))


def plan(scans: Sequence[ModelScan]):
    """(header rows int64[K, 8], per scan the five parts as uint8 arrays) by the rules of gf_pk_pack_device."""
    rows = np.zeros((len(scans), 8), dtype=np.int64)
    parts = []
    for i, s in enumerate(scans):
        t, nt = s.totals, s.name_totals
        hits_cap, bytes_cap, names_cap = s.hits.shape[0], min(s.bases.size, s.quals.size), s.names.size
        bits = int(t[4]) & (OVER_RETRY | OVER_HITS)
        if int(nt[2]) & 1:
            bits |= OVER_NAMES
        rec, rb, nb = _clamp(t[0], hits_cap), _clamp(t[1], bytes_cap), _clamp(nt[1], names_cap)
        first = int(s.name_off[0])
        if not bits and (rec != t[0] or rb != t[1] or nb != nt[1] or nt[0] != rec or first < 0 or first > names_cap - nb):
            bits = BAD_SCAN
        if bits:
            rec = rb = nb = 0
        rows[i] = (rec, rb, nb, t[2], t[3], t[0], nt[3], bits | (max(int(nt[1]), 0) << 8))
        off = np.empty(0, dtype=np.int64) if bits else s.name_off[:rec + 1] - first
        parts.append([s.hits[:rec].reshape(-1), s.bases[:rb], s.quals[:rb], off.astype("<i8").view(np.uint8),
                      s.names[first:first + nb] if nb else np.empty(0, dtype=np.uint8)])
    return rows, parts


def pack_model(scans: Sequence[ModelScan], block_bytes: Optional[int] = None) -> bytes:
    """The block of ``scans``: the headers and the body; with a ``block_bytes`` smaller than that, the headers alone,
    the overflow flag set."""
    k = len(scans)
    rows, parts = plan(scans)
    body = bytearray()
    for c in range(len(SECTIONS)):
        for p in parts:
            body += p[c].tobytes()
        body += bytes(-len(body) % 16)
    need = 64 * (k + 1) + len(body)
    over = block_bytes is not None and block_bytes < need
    head = np.zeros((k + 1, 8), dtype=np.int64)
    head[0, :3] = (len(body), k, int(over))
    head[1:] = rows
    return head.tobytes() + (b"" if over else bytes(body))


def piece_kinds(scans: Sequence[ModelScan], aligns: Sequence[dict]) -> dict:
    """How many aligned 16-byte pieces of the body are of each kind: ``aligned`` (inside one part whose source lies on
    the destination's 16-byte grid), ``bytewise`` (inside one part, the source off the grid), ``straddle`` (over two
    or more parts, or a part and the section's padding), ``offsets`` (the name offsets' section).  ``aligns[i]``: per
    section name, the address of scan i's source modulo 16."""
    _, parts = plan(scans)
    kinds = {"aligned": 0, "bytewise": 0, "straddle": 0, "offsets": 0}
    for c, sec in enumerate(SECTIONS):
        lens = [p[c].size for p in parts]
        total = sum(lens)
        if sec == "offsets":
            kinds["offsets"] += (total + 15) // 16
            continue
        ends = np.cumsum(lens)
        starts = ends - lens
        d0 = np.arange(0, total, 16)
        i = np.searchsorted(ends, d0, side="right")   # the part byte d0 lies in (empty ones stepped over)
        straddle = d0 + 16 > ends[i]
        on_grid = (np.array([a[sec] for a in aligns])[i] + d0 - starts[i]) % 16 == 0
        kinds["straddle"] += int(straddle.sum())
        kinds["aligned"] += int((~straddle & on_grid).sum())
        kinds["bytewise"] += int((~straddle & ~on_grid).sum())
    return kinds


def same_scans(unpacked, scans: Sequence[ModelScan]) -> None:
    """What ``scan_pack.unpack_block`` gave is what the scans hold, scan by scan."""
    rows, parts = plan(scans)
    assert len(unpacked) == len(scans)
    for u, s, row, p in zip(unpacked, scans, rows, parts):
        assert u.rec.tobytes() == p[0].tobytes() and u.bases == p[1].tobytes() and u.quals == p[2].tobytes()
        off = p[3].view("<i8")
        assert u.names == [p[4].tobytes()[off[j]:off[j + 1]] for j in range(int(row[0]))]
        assert u.bits == int(row[7]) & 255 and u.name_bytes == int(row[7]) >> 8 and u.missing == int(s.name_totals[3])
        assert u.totals == {"hits": int(s.totals[0]), "hit_bytes": int(row[1]), "merged_pairs": int(s.totals[2]),
                            "retried_reads": int(s.totals[3]), "overflow": int(row[7]) & 255}
