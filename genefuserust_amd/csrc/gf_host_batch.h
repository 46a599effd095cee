// Host side of the host-buffer calls (gf_map_reads, gf_map_reads_hits, gf_stream_submit, gf_stream_submit_packed): the
// one check of a pack's offsets, and where its pieces lie in the device arena of a staged batch and in the pinned block
// of a zero-copy call.  Plain C++, no HIP: tests/cpp/test_host_batch.cpp holds it to a model under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/gfmatch.h"

static inline size_t gf_hb_up(size_t x, size_t a) { return (x + a - 1) & ~(a - 1); }

// a pack: n reads, the longest of maxlen bases, in [b0, b1) = [offsets[0], offsets[n]) of the caller's buffer, gaps included
struct gf_pack_span { int64_t n = 0, b0 = 0, b1 = 0, maxlen = 0; };

// The one check, the offsets' half: n, the pointer, non-decreasing offsets (a decrease anywhere is GF_ERR_ARG, even
// behind a read that is too long), no read beyond GF_MAX_READ_LEN.
static inline int gf_pack_measure(const int64_t* offsets, int64_t n, gf_pack_span* p) {
  if (n < 0 || (n > 0 && !offsets)) return GF_ERR_ARG;
  int64_t maxlen = 0;
  for (int64_t r = 0; r < n; ++r) {
    const int64_t l = offsets[r + 1] - offsets[r];
    if (l < 0) return GF_ERR_ARG;
    if (l > maxlen) maxlen = l;
  }
  if (maxlen > GF_MAX_READ_LEN) return GF_ERR_READ_TOO_LONG;
  *p = {n, n > 0 ? offsets[0] : 0, n > 0 ? offsets[n] : 0, maxlen};  // (a refused pack leaves *p as it was)
  return GF_OK;
}
// The reads' half: a span that holds bases needs them.  (The stream entries ask about capacity between the two halves.)
static inline int gf_pack_reads_present(const gf_pack_span& p, bool have_reads) {
  return p.b1 > p.b0 && !have_reads ? GF_ERR_ARG : GF_OK;
}

// The staged batch, | bases | offsets | counts | matches | hits | total | compaction workspace |: byte offsets into one
// device block of `bytes`, every region a multiple of 256 bytes.  The bases region takes an ASCII span at the 16-byte
// phase of its host address (the kernels stage whole chunks) or its packed chunks; 64 bytes of slack for either.
// compact_ws_bytes: gf_compact_workspace_bytes(reads), which the kernels' tile size decides.
struct gf_staged_layout { size_t bases, offsets, counts, matches, hits, total, compact_ws, bytes; };
static inline gf_staged_layout gf_staged_layout_for(int64_t reads, int64_t bytes, int64_t hits_cap, int64_t compact_ws_bytes) {
  const size_t n = (size_t)reads;
  gf_staged_layout a{};  // (bases at 0)
  a.offsets = a.bases + gf_hb_up((size_t)bytes + 64, 256);
  a.counts = a.offsets + gf_hb_up((n + 1) * sizeof(int64_t), 256);
  a.matches = a.counts + gf_hb_up(n + 1, 256);
  a.hits = a.matches + gf_hb_up((n * 2 + 1) * sizeof(gf_seqmatch), 256);
  a.total = a.hits + gf_hb_up(((size_t)hits_cap + 1) * sizeof(gf_hit), 256);
  a.compact_ws = a.total + 256;
  a.bytes = a.compact_ws + gf_hb_up((size_t)compact_ws_bytes + 16, 256);
  return a;
}

// The packed form of the span [b0, b1) in the bases region: chunks c0 .. c0+nc-1 of the caller's stream cover the
// pack's bases and the four chunks past them that every packed buffer carries (gf_packed_chunks: the kernels' staging
// reads past a tile's last chunk; the host's arrays hold them — the next reads' chunks inside a buffer,
// gf_pack_bases_host's padding at its end): nc words of pk at the region's start, nc half-words of iv at `iv_at`,
// 6 bytes per chunk of 16 bases.  A stream slot's region (max_bytes + 64 bytes) holds a pack whose `bytes` fit in it.
struct gf_packed_stage { int64_t c0, nc; size_t iv_at, bytes; };
static inline gf_packed_stage gf_packed_stage_for(int64_t b0, int64_t b1) {
  const int64_t c0 = b0 >> 4, nc = ((b1 + 15) >> 4) + 4 - c0;
  const size_t iv_at = gf_hb_up((size_t)nc * 4, 16);
  return {c0, nc, iv_at, iv_at + (size_t)nc * 2};
}

// A zero-copy call's pinned block, | completion word (64 B) | offsets | matches | counts | bases |, in 16-byte granules.
// `staged`: the reads are copied into the block; reads that lie in a gf_host_alloc block are read where they are and
// take no room here.  bytes: what to reserve, the regions and 64 bytes of slack.
struct gf_zc_layout { size_t offsets, matches, counts, bases, bytes; };
static inline gf_zc_layout gf_zc_layout_for(int64_t n, int64_t bytes, bool staged) {
  gf_zc_layout z;
  z.offsets = 64;
  z.matches = z.offsets + gf_hb_up(((size_t)n + 1) * sizeof(int64_t), 16);
  z.counts = z.matches + (size_t)n * 2 * sizeof(gf_seqmatch);
  z.bases = z.counts + gf_hb_up((size_t)n, 16);
  z.bytes = z.bases + (staged ? gf_hb_up((size_t)bytes + 64, 16) : 0) + 64;
  return z;
}
