// The gene slices of a reference FASTA, cut from a chunk of its text in HBM (include/gf_ref_cut.h):
//
//   gf_rc_index_device
//     '>' and kept bytes (letters, '-', '*') per tile                   gf_rc_k_count (a thread per 16-byte piece)
//     where each tile's records and kept bytes start; the totals        gf_rc_k_scan (one block)
//     the '>' positions in ascending order, the kept rank at each       gf_rc_k_scatter (a thread per piece)
//     each record's name delimiter and the rank at its sequence start   gf_rc_k_names (a wavefront per record)
//     where each name goes: an exclusive scan of the lengths            gf_rc_k_name_scan (one block, in place)
//     the names, back to back                                           gf_rc_k_name_copy (a wavefront per name)
//   gf_rc_gather_device
//     the kept bytes of the wanted ranges, upper-cased                  gf_rc_k_gather (a thread per piece)
//
// A piece is an aligned 16-byte block of addresses, a tile GF_RC_THREADS of them: the text may start anywhere, so the
// tiles lie on the grid of addresses and the bytes of the first and last piece that are not text are masked out.  An
// aligned block that holds one byte of an allocation lies in the allocation's page, so the whole of it may be loaded.
// Deterministic: tile counts -> scan -> scatter, no atomics.
#pragma once

#include "../../include/gf_ref_cut.h"
#include "gf_scan_common.h"

#define GF_RC_THREADS GF_SCAN_THREADS
#define GF_RC_PIECE 16
#define GF_RC_TILE (GF_RC_THREADS * GF_RC_PIECE)

// the text on the grid of addresses: byte p of the text is base[head + p], base a multiple of 16, head 0 .. 15
struct GfRcText {
  const uint8_t* base;
  int64_t head, n;
};

__device__ __forceinline__ bool gf_rc_keep(uint32_t c) { return ((c | 0x20u) - 'a') < 26u || c == '-' || c == '*'; }
__device__ __forceinline__ bool gf_rc_delim(uint32_t c) { return c == '\n' || c == ' '; }

// the thread's piece of the block's tile: its bytes (w, byte j of the piece in bits 8 (j & 3) of w[j >> 2]) and which
// of them are '>' / kept, text bytes only; a: where the piece starts on the grid (byte j is text byte a + j - head)
struct GfRcPiece {
  uint32_t w[4];
  uint32_t gt, keep, valid;
  int64_t a;
};

__device__ __forceinline__ GfRcPiece gf_rc_load_piece(const GfRcText& T) {
  GfRcPiece P;
  P.a = (int64_t)blockIdx.x * GF_RC_TILE + (int64_t)threadIdx.x * GF_RC_PIECE;
  const int64_t lo = T.head - P.a, hi = T.head + T.n - P.a;  // the text's bytes of the piece: [lo, hi) of 0 .. 16
  P.gt = P.keep = P.valid = 0;
  P.w[0] = P.w[1] = P.w[2] = P.w[3] = 0;
  if (hi <= 0 || lo >= GF_RC_PIECE) return P;
  const uint32_t below_hi = hi >= GF_RC_PIECE ? 0xffffu : (1u << hi) - 1u;
  const uint32_t below_lo = lo <= 0 ? 0u : (1u << lo) - 1u;
  P.valid = below_hi & ~below_lo;
  const uint4 q = *(const uint4*)(T.base + P.a);
  P.w[0] = q.x; P.w[1] = q.y; P.w[2] = q.z; P.w[3] = q.w;
#pragma unroll
  for (int j = 0; j < GF_RC_PIECE; ++j) {
    const uint32_t c = (P.w[j >> 2] >> (8 * (j & 3))) & 0xffu;
    P.gt |= (uint32_t)(c == '>') << j;
    P.keep |= (uint32_t)gf_rc_keep(c) << j;
  }
  P.gt &= P.valid;
  P.keep &= P.valid;
  return P;
}

// ---- count: the tile's '>' and kept bytes
__global__ __launch_bounds__(GF_RC_THREADS) void gf_rc_k_count(GfRcText T, uint32_t* __restrict__ tile_gt,
                                                               uint32_t* __restrict__ tile_keep) {
  __shared__ int s_a[GF_RC_THREADS / 64];
  __shared__ long long s_b[GF_RC_THREADS / 64];
  const GfRcPiece P = gf_rc_load_piece(T);
  int ea, ta;
  long long eb, tb;
  gf_scan_block_scan2(__popc(P.gt), (long long)__popc(P.keep), s_a, s_b, ea, eb, ta, tb);
  if (threadIdx.x == 0) {
    tile_gt[blockIdx.x] = (uint32_t)ta;
    tile_keep[blockIdx.x] = (uint32_t)tb;
  }
}

// ---- scan: the tiles' counts to exclusive offsets (tile_gt_off[0 .. ntiles), tile_kept[0 .. ntiles]) and the totals.
// One block, both sequences in one pass (gf_scan_totals_block).
__global__ __launch_bounds__(GF_SCAN_TOTALS_THREADS) void gf_rc_k_scan(
    const uint32_t* __restrict__ tile_gt, const uint32_t* __restrict__ tile_keep, int64_t ntiles, int64_t cap_records,
    int64_t* __restrict__ tile_gt_off, int64_t* __restrict__ tile_kept, int64_t* __restrict__ totals) {
  const uint32_t* const in[2] = {tile_gt, tile_keep};
  int64_t* const out[2] = {tile_gt_off, tile_kept};
  long long total[2];
  gf_scan_totals_block(in, out, ntiles, total);
  const long long tg = total[0], tk = total[1];
  if (threadIdx.x == 0) {
    tile_kept[ntiles] = tk;
    totals[0] = tg;
    totals[1] = tk;
    totals[2] = tg > cap_records ? 1 : 0;
    totals[3] = -1;  // (gf_rc_k_names knows better)
    totals[4] = 0;
  }
}

// ---- scatter: record k's '>' position and the kept rank there, k ascending with the position
__global__ __launch_bounds__(GF_RC_THREADS) void gf_rc_k_scatter(GfRcText T, const int64_t* __restrict__ tile_gt_off,
                                                                 const int64_t* __restrict__ tile_kept,
                                                                 int64_t cap_records, int64_t* __restrict__ gt_pos,
                                                                 int64_t* __restrict__ gt_rank) {
  __shared__ int s_a[GF_RC_THREADS / 64];
  __shared__ long long s_b[GF_RC_THREADS / 64];
  const GfRcPiece P = gf_rc_load_piece(T);
  int ea, ta;
  long long eb, tb;
  gf_scan_block_scan2(__popc(P.gt), (long long)__popc(P.keep), s_a, s_b, ea, eb, ta, tb);
  uint32_t gt = P.gt;
  if (!gt) return;
  int64_t k = tile_gt_off[blockIdx.x] + ea;
  const int64_t rank0 = tile_kept[blockIdx.x] + eb;
  while (gt && k < cap_records) {
    const int j = __builtin_ctz(gt);
    gt &= gt - 1;
    gt_pos[k] = P.a + j - T.head;
    gt_rank[k] = rank0 + __popc(P.keep & ((1u << j) - 1u));
    ++k;
  }
}

__device__ __forceinline__ int64_t gf_rc_known(const int64_t* __restrict__ totals, int64_t cap_records) {
  const int64_t n = totals[0];
  return n < cap_records ? n : cap_records;
}

// ---- names: record k by one wavefront, 64 bytes a step from the byte after its '>' to the first delimiter, the next
// '>' or the end of the text.  name_off[k] = the name's length (scanned in place by gf_rc_k_name_scan).
__global__ __launch_bounds__(GF_RC_THREADS) void gf_rc_k_names(GfRcText T, const int64_t* __restrict__ gt_pos,
                                                               const int64_t* __restrict__ gt_rank,
                                                               int64_t cap_records, int64_t* __restrict__ name_end,
                                                               int64_t* __restrict__ seq_rank,
                                                               int64_t* __restrict__ name_off,
                                                               int64_t* __restrict__ totals) {
  const int64_t n = gf_rc_known(totals, cap_records);
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (GF_RC_THREADS / 64);
  const uint8_t* __restrict__ text = T.base + T.head;
  for (int64_t k = (int64_t)blockIdx.x * (GF_RC_THREADS / 64) + (threadIdx.x >> 6); k < n; k += waves) {
    const int64_t g = gt_pos[k];
    const int64_t end = k + 1 < n ? gt_pos[k + 1] : T.n;
    int64_t kept = 0, at = -1;
#pragma unroll 1
    for (int64_t b = g + 1; b < end; b += 64) {
      const bool in = b + lane < end;
      const uint32_t c = in ? text[b + lane] : 0u;
      const uint64_t dm = __ballot(in && gf_rc_delim(c));
      const uint64_t km = __ballot(in && gf_rc_keep(c));
      if (dm) {
        const int f = __builtin_ctzll(dm);
        kept += __popcll(km & ((1ull << f) - 1ull));
        at = b + f;
        break;
      }
      kept += __popcll(km);
    }
    if (lane == 0) {
      name_end[k] = at;
      seq_rank[k] = gt_rank[k] + kept;
      name_off[k] = (at < 0 ? end : at) - g - 1;
      if (at < 0 && k + 1 == totals[0]) totals[3] = g;  // the last record of the chunk, its header unfinished
    }
  }
}

// ---- name scan: name_off[0 .. n) from lengths to exclusive offsets, name_off[n] the total (as gf_hn_k_scan)
__global__ __launch_bounds__(GF_SCAN_TOTALS_THREADS) void gf_rc_k_name_scan(int64_t cap_records, int64_t names_cap,
                                                                            int64_t* __restrict__ off,
                                                                            int64_t* __restrict__ totals) {
  const int64_t n = gf_rc_known(totals, cap_records);
  const long long total = gf_scan_totals_block(off, off, n);
  if (threadIdx.x == 0) {
    off[n] = total;
    totals[4] = total;
    if (total > names_cap) totals[2] |= 2;
  }
}

// ---- name copy: name k by the 64 lanes of one wavefront; a name that does not fit names_cap is not written at all
__global__ __launch_bounds__(GF_RC_THREADS) void gf_rc_k_name_copy(GfRcText T, const int64_t* __restrict__ gt_pos,
                                                                   const int64_t* __restrict__ off,
                                                                   const int64_t* __restrict__ totals,
                                                                   int64_t cap_records, uint8_t* __restrict__ names,
                                                                   int64_t names_cap) {
  const int64_t n = gf_rc_known(totals, cap_records);
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (GF_RC_THREADS / 64);
  const uint8_t* __restrict__ text = T.base + T.head;
  for (int64_t k = (int64_t)blockIdx.x * (GF_RC_THREADS / 64) + (threadIdx.x >> 6); k < n; k += waves) {
    const int64_t o = off[k], len = off[k + 1] - o, g = gt_pos[k];
    if (len <= 0 || o + len > names_cap || g + 1 + len > T.n) continue;
    const uint8_t* __restrict__ src = text + g + 1;
#pragma unroll 1
    for (int64_t j = lane; j < len; j += 64) names[o + j] = src[j];
  }
}

// ---- gather.  The first interval that ends behind position pos of record r: intervals are disjoint and sorted by
// (record, start), so by (record, end) too.
__device__ __forceinline__ int64_t gf_rc_find_interval(const gf_rc_interval* __restrict__ iv, int64_t m, int64_t r,
                                                       int64_t pos) {
  int64_t lo = 0, hi = m;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const int64_t rec = iv[mid].record;
    if (rec < r || (rec == r && iv[mid].end <= pos)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// A thread per piece: its kept rank from the tile's (gf_rc_index_device wrote it) and the block's scan, its record by a
// binary search over the '>' positions, the interval by another over the record's intervals.  A piece of one record
// that touches no interval — nearly all of a genome — ends there: one load, no store.
__global__ __launch_bounds__(GF_RC_THREADS) void gf_rc_k_gather(GfRcText T, const int64_t* __restrict__ gt_pos,
                                                                const int64_t* __restrict__ seq_rank, int64_t n,
                                                                const int64_t* __restrict__ tile_kept,
                                                                int64_t carried_kept,
                                                                const gf_rc_interval* __restrict__ iv, int64_t m,
                                                                uint8_t* __restrict__ out, int64_t out_cap) {
  __shared__ int s_a[GF_RC_THREADS / 64];
  __shared__ long long s_b[GF_RC_THREADS / 64];
  const GfRcPiece P = gf_rc_load_piece(T);
  int ea, ta;
  long long eb, tb;
  gf_scan_block_scan2(0, (long long)__popc(P.keep), s_a, s_b, ea, eb, ta, tb);
  if (!P.keep) return;
  // the record the piece starts in: the number of '>' in front of its first text byte
  const int64_t first = P.a + __builtin_ctz(P.valid) - T.head;
  int64_t r = 0;
  {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (gt_pos[mid] < first) lo = mid + 1;
      else hi = mid;
    }
    r = lo;
  }
  int64_t rank = tile_kept[blockIdx.x] + eb;
  int64_t base = r == 0 ? -carried_kept : seq_rank[r - 1];
  int64_t i = -1;  // the interval search of record r is still to do
  if (!P.gt) {
    const int64_t lo = rank - base, hi = lo + __popc(P.keep);
    if (hi <= 0) return;  // name bytes
    i = gf_rc_find_interval(iv, m, r, lo < 0 ? 0 : lo);
    if (i >= m || iv[i].record != r || iv[i].start >= hi) return;
  }
  uint32_t w0 = P.w[0], w1 = P.w[1], w2 = P.w[2], w3 = P.w[3];
  uint32_t gt = P.gt, keep = P.keep;
#pragma unroll 1
  for (int j = 0; j < GF_RC_PIECE && (gt | keep); ++j) {
    const uint32_t c = w0 & 0xffu;
    w0 = (w0 >> 8) | (w1 << 24); w1 = (w1 >> 8) | (w2 << 24); w2 = (w2 >> 8) | (w3 << 24); w3 >>= 8;
    const bool is_gt = gt & 1u, is_keep = keep & 1u;
    gt >>= 1;
    keep >>= 1;
    if (is_gt) {
      if (++r > n) return;  // (a record the caller does not know of: nothing of it is wanted)
      base = seq_rank[r - 1];
      i = -1;
    } else if (is_keep) {
      const int64_t pos = rank - base;
      ++rank;
      if (pos < 0) continue;
      if (i < 0) i = gf_rc_find_interval(iv, m, r, pos);
      while (i < m && iv[i].record == r && iv[i].end <= pos) ++i;
      if (i >= m || iv[i].record != r || iv[i].start > pos) continue;
      const int64_t o = iv[i].out_offset + pos - iv[i].start;
      if (o >= 0 && o < out_cap) out[o] = (uint8_t)(c >= 'a' ? c - 0x20u : c);
    }
  }
}
