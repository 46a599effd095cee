"""The host-buffer calls on both of their routes (needs a GPU): gf_map_reads, gf_map_reads_hits, gf_stream_submit and
gf_stream_submit_packed share one pack check, one staged arena and one queued batch route
(genefuserust_amd/csrc/gf_host_batch.h, gfmatch.hip "host-buffer entry points").  Held here: the code each entry
returns for a refused pack, that lane and stream are as usable after a refusal as before it, and that ASCII and packed
packs may share the slots of one stream.  Packs of 3 reads take the small zero-copy route whatever the setting; packs of
70 take the pack zero-copy route by default and the batch route after set_pack_call_reads(0).
(The file sorts behind the other GPU tests for the reason tests/test_whole_genome_alignable_gpu.py gives.)"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L, PACK, N_PACKS, SEED = 150, 70, 7, 8     # the seed: chosen with the oracle, see `world`
MAX_READ_LEN = 4096


@pytest.fixture(scope="module")
def world(gpu_device):
    from genefuserust_amd import Indexer, synth
    from genefuserust_amd.stream import pack_bases_host
    from oracle import oracle_py
    genes = synth.make_geneset("IDX-T", scale=0.02)
    synth.MIXES["TEST"] = (0.2, 0.5, 0.3)
    rb = synth.make_reads(genes, PACK * N_PACKS, read_len=L, mix="TEST", seed=SEED)
    bases, offsets = rb.bases.numpy(), rb.offsets.numpy()
    counts, _ = oracle_py.OracleIndexer(genes.seqs).map_reads_packed(bases, offsets)
    hit = counts > 0
    # every pack used below holds a read with a match and a read without
    assert 0 < hit[:3].sum() < 3 and all(0 < hit[k:k + PACK].sum() < PACK for k in range(0, hit.size, PACK))
    ix = Indexer.from_gene_slices(genes.seqs, genes.reversed_flags)
    ix.make_index()
    pk, iv = pack_bases_host(bases)
    yield dict(ix=ix, bases=bases, offsets=offsets, pk=pk, iv=iv, hit=hit)
    ix.set_pack_call_reads(-1)
    ix.close()


class Raw:
    """The four entries through _lib.lib() itself: (code, output bytes).  A stream of `depth` slots opened for exactly
    `n` reads of L bases; submit and collect are separate so that a test can fill its slots."""

    def __init__(self, w, n, depth=2):
        from genefuserust_amd import _lib
        self.lib, self.codes, self.w, self.n, self.depth = _lib.lib(), _lib, w, n, depth
        self.h = w["ix"]._handle()
        self.stream = C.c_void_p()
        _lib.check(self.lib.gf_stream_open(self.h, n, n * L, depth, C.byref(self.stream)))

    def close(self):
        self.lib.gf_stream_close(self.stream)

    def map_reads(self, off, n):
        from genefuserust_amd._lib import SEQMATCH_DTYPE
        counts, matches = np.zeros(max(n, 1), dtype=np.int32), np.zeros((max(n, 1), 2), dtype=SEQMATCH_DTYPE)
        rc = self.lib.gf_map_reads(self.h, self.w["bases"].ctypes.data, off.ctypes.data, n, counts.ctypes.data,
                                   matches.ctypes.data)
        return rc, counts.tobytes() + matches.tobytes()

    def map_reads_hits(self, off, n):
        from genefuserust_amd._lib import HIT_DTYPE
        hits, total = np.zeros(max(n, 1), dtype=HIT_DTYPE), C.c_int64(0)
        rc = self.lib.gf_map_reads_hits(self.h, self.w["bases"].ctypes.data, off.ctypes.data, n, 77, hits.ctypes.data,
                                        hits.size, C.byref(total))
        return rc, hits[:max(0, min(int(total.value), hits.size))].tobytes()

    def submit(self, off, n):
        return self.lib.gf_stream_submit(self.stream, self.w["bases"].ctypes.data, off.ctypes.data, n, 77)

    def submit_packed(self, off, n):
        return self.lib.gf_stream_submit_packed(self.stream, self.w["pk"].ctypes.data, self.w["iv"].ctypes.data,
                                                off.ctypes.data, n, 77)

    def collect(self):
        from genefuserust_amd._lib import HIT_DTYPE
        hits, total = np.zeros(self.n + 1, dtype=HIT_DTYPE), C.c_int64(0)
        rc = self.lib.gf_stream_collect(self.stream, hits.ctypes.data, hits.size, C.byref(total))
        return rc, hits[:max(0, min(int(total.value), hits.size))].tobytes()

    def call(self, entry, off, n):
        if entry in ("gf_map_reads", "gf_map_reads_hits"):
            return getattr(self, entry[3:])(off, n)
        rc = getattr(self, entry[10:])(off, n)
        return (rc, b"") if rc != 0 else self.collect()


ENTRIES = ("gf_map_reads", "gf_map_reads_hits", "gf_stream_submit", "gf_stream_submit_packed")


@pytest.mark.parametrize("n", [3, PACK])
@pytest.mark.parametrize("route", [-1, 0])
@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_leave_lane_and_stream_usable(world, entry, route, n):
    from genefuserust_amd import _lib
    ix, offsets = world["ix"], world["offsets"]
    good = np.ascontiguousarray(offsets[:n + 1])
    decreasing = good.copy()
    decreasing[(n + 1) // 2] = decreasing[(n + 1) // 2 - 1] - 1
    too_long = good.copy()
    too_long[n] = too_long[n - 1] + MAX_READ_LEN + 1
    refused = [(decreasing, n, _lib.GF_ERR_ARG), (too_long, n, _lib.GF_ERR_READ_TOO_LONG)]
    if "stream" in entry:
        too_many = np.ascontiguousarray(offsets[:n + 2])          # n = max_reads + 1
        too_wide = good.copy()
        too_wide[n] = too_wide[0] + n * L + 1                     # a span of max_bytes + 1
        refused += [(too_many, n + 1, _lib.GF_ERR_CAPACITY), (too_wide, n, _lib.GF_ERR_CAPACITY)]
    raw = Raw(world, n)
    try:
        ix.set_pack_call_reads(route)
        rc, want = raw.call(entry, good, n)
        assert rc == 0
        if entry != "gf_map_reads":
            assert len(want) == 48 * int(world["hit"][:n].sum())
        for off, k, code in refused:
            assert raw.call(entry, off, k)[0] == code, (k, code)
            assert raw.call(entry, good, n) == (0, want), (k, code)
        if "stream" in entry:      # every slot in flight: the next submit is refused, the packs in flight collect intact
            submit = getattr(raw, entry[10:])
            assert [submit(good, n) for _ in range(raw.depth + 1)] == [0] * raw.depth + [_lib.GF_ERR_CAPACITY]
            assert [raw.collect() for _ in range(raw.depth)] == [(0, want)] * raw.depth
            assert raw.call(entry, good, n) == (0, want)
    finally:
        ix.set_pack_call_reads(-1)
        raw.close()


@pytest.mark.parametrize("route", [-1, 0])
def test_ascii_and_packed_packs_share_a_stream(world, route):
    """Two slots, seven packs of 70 reads and an empty one, submitted ASCII, ASCII, packed, packed, ASCII, ASCII, empty,
    packed: slot 0 carries ASCII, packed, ASCII, (empty), slot 1 ASCII, packed, ASCII, packed — both kinds in both
    orders on either.  A packed pack once kept the `zc_call` of the ASCII pack its slot carried before and was
    collected as that pack."""
    from genefuserust_amd.stream import MapStream
    ix, bases, offsets, pk, iv = (world[k] for k in ("ix", "bases", "offsets", "pk", "iv"))
    kinds = ["ascii", "ascii", "packed", "packed", "ascii", "ascii", "empty", "packed"]
    got, inflight, p = [], 0, 0
    try:
        ix.set_pack_call_reads(route)
        want = ix.map_reads_hits(bases, offsets, read_id_base=1000)
        assert want.shape[0] == int(world["hit"].sum())
        with MapStream(ix, max_reads=PACK, max_bytes=PACK * L, depth=2) as ms:
            for kind in kinds:
                if inflight == ms.depth:
                    got.append(ms.collect())
                    inflight -= 1
                if kind == "empty":
                    ms.submit(bases, offsets[p * PACK:p * PACK + 1], read_id_base=5)
                else:
                    off = offsets[p * PACK:(p + 1) * PACK + 1]
                    if kind == "ascii":
                        ms.submit(bases, off, read_id_base=1000 + p * PACK)
                    else:
                        ms.submit_packed(pk, iv, off, read_id_base=1000 + p * PACK)
                    p += 1
                inflight += 1
            while inflight:
                got.append(ms.collect())
                inflight -= 1
    finally:
        ix.set_pack_call_reads(-1)
    assert p == N_PACKS and len(got) == len(kinds) and got[kinds.index("empty")].shape[0] == 0
    assert np.concatenate(got).tobytes() == want.tobytes()
