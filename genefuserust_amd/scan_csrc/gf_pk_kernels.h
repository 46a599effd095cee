// The outputs of K scans and their names, packed into one block (include/gf_scan_pack.h):
//
//   what each scan really holds, where each part goes, the headers    gf_pk_k_plan (one block)
//   the body, in aligned 16-byte pieces of the block                  gf_pk_k_copy
//
// The body is five sections (records, bases, qualities, name offsets, names), each the K scans' parts back to back
// and then zeros up to the next 16-byte boundary.  The plan kernel writes the start of every part into the workspace
// as one ascending list of 5 (K + 1) entries — per section the K parts and the section's padding — closed by the
// body's size; the copy kernel holds that list in LDS, and a piece finds the part it starts in by binary search.
// Deterministic: no atomics.
#pragma once

#include "../../include/gf_scan_pack.h"
#include "gf_scan_common.h"

#define GF_PK_PIECE 16           // bytes a thread of gf_pk_k_copy moves at a time: one aligned 16-byte store
#define GF_PK_COPY_BLOCKS 1024   // the cap of gf_pk_k_copy's grid; the blocks stride over the pieces
#define GF_PK_SECTIONS 5
#define GF_PK_SEC_OFFSETS 3      // (0 records, 1 bases, 2 qualities, 3 name offsets, 4 names)
#define GF_PK_HEADER_BYTES(k) (64 * ((int64_t)(k) + 1))
#define GF_PK_ENTRIES(k) (GF_PK_SECTIONS * ((k) + 1))

__device__ __forceinline__ int64_t gf_pk_clamp(int64_t v, int64_t cap) { return v < 0 ? 0 : (v < cap ? v : cap); }

// ---- plan: thread i reads scan i's totals and clamps them; the five sequences of part lengths are scanned to starts
// (gf_scan_totals_block, in place in the workspace, one after the other); the headers.
// start: int64[GF_PK_ENTRIES(k) + 1].
__global__ __launch_bounds__(GF_SCAN_TOTALS_THREADS) void gf_pk_k_plan(const gf_pk_scan* __restrict__ scans, int k,
                                                                      int64_t* start, int64_t* __restrict__ block,
                                                                      int64_t block_bytes) {
  const int i = threadIdx.x;
  int64_t rec = 0, rb = 0, nb = 0;
  if (i < k) {
    const gf_pk_scan s = scans[i];
    const int64_t* t = (const int64_t*)s.d_totals;
    const int64_t* nt = (const int64_t*)s.d_name_totals;
    int64_t hits = 0, merged = 0, retried = 0, missing = 0, name_bytes = 0;
    int64_t bits = 0;
    if (!t || !nt || !s.d_name_off || s.hits_cap < 0 || s.bytes_cap < 0 || s.names_cap < 0) {
      bits = GF_PK_BAD_SCAN;
      if (t) hits = t[0];
    } else {
      hits = t[0]; merged = t[2]; retried = t[3];
      missing = nt[3];
      name_bytes = nt[1] < 0 ? 0 : nt[1];
      bits = t[4] & (GF_PK_OVER_RETRY | GF_PK_OVER_HITS);
      if (nt[2] & 1) bits |= GF_PK_OVER_NAMES;
      rec = gf_pk_clamp(hits, s.hits_cap);
      rb = gf_pk_clamp(t[1], s.bytes_cap);
      nb = gf_pk_clamp(nt[1], s.names_cap);
      const int64_t first = ((const int64_t*)s.d_name_off)[0];
      if (!bits && (rec != hits || rb != t[1] || nb != nt[1] || nt[0] != rec || (rec > 0 && !s.d_hits) ||
                    (rb > 0 && (!s.d_bases || !s.d_quals)) || (nb > 0 && !s.d_names) || first < 0 ||
                    first > s.names_cap - nb))
        bits = GF_PK_BAD_SCAN;
    }
    if (bits) rec = rb = nb = 0;
    const int64_t len[GF_PK_SECTIONS] = {rec * (int64_t)sizeof(gf_pair_hit), rb, rb, bits ? 0 : 8 * (rec + 1), nb};
#pragma unroll
    for (int c = 0; c < GF_PK_SECTIONS; ++c) start[c * (k + 1) + i] = len[c];
    int64_t* h = block + 8 + 8 * (int64_t)i;
    h[0] = rec; h[1] = rb; h[2] = nb; h[3] = merged; h[4] = retried; h[5] = hits; h[6] = missing;
    h[7] = bits | (name_bytes << 8);
  }
  __syncthreads();  // (a thread of the scan below reads lengths that other threads stored)
  // (one sequence at a time: five at once would not fit the registers of a 1024-thread block)
  int64_t base = 0;
#pragma unroll 1
  for (int c = 0; c < GF_PK_SECTIONS; ++c) {
    int64_t* seq = start + c * (k + 1);
    const int64_t total = gf_scan_totals_block(seq, seq, (int64_t)k);
    __syncthreads();  // (the starts within the section are stored, and the scan's LDS is free for the next one)
    if (i < k) seq[i] += base;  // the section lies behind the one before it
    if (i == 0) seq[k] = base + total;  // the section's padding
    base += (total + GF_PK_PIECE - 1) & ~(int64_t)(GF_PK_PIECE - 1);
  }
  if (i == 0) {
    const int64_t body = base;
    start[GF_PK_ENTRIES(k)] = body;
    block[0] = body;
    block[1] = k;
    block[2] = GF_PK_HEADER_BYTES(k) + body > block_bytes ? 1 : 0;
    block[3] = block[4] = block[5] = block[6] = block[7] = 0;
  }
}

// where part (section c, scan sc) comes from
__device__ __forceinline__ const uint8_t* gf_pk_source(const gf_pk_scan* __restrict__ scans, int c, int sc) {
  const gf_pk_scan& s = scans[sc];
  switch (c) {
    case 0: return (const uint8_t*)s.d_hits;
    case 1: return (const uint8_t*)s.d_bases;
    case 2: return (const uint8_t*)s.d_quals;
    case GF_PK_SEC_OFFSETS: return (const uint8_t*)s.d_name_off;
    default: return (const uint8_t*)s.d_names + ((const int64_t*)s.d_name_off)[0];
  }
}

// ---- copy: a thread takes one aligned 16-byte piece of the body at a time and finds the part the piece starts in by
// binary search over the starts in LDS.  A piece that lies inside one part whose source is on the same 16-byte grid —
// nearly all of them, the scans' buffers being allocated aligned — is one 16-byte load; any other piece is put
// together byte by byte, stepping from part to part as gf_mc_k_gather does (empty parts are stepped over, a section's
// padding gives zeros).  The name offsets go as two int64 per piece, each less its scan's first offset.  The volume is
// the hits of one chunk — kilobytes to a few megabytes — so nothing here is tuned beyond that.
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_pk_k_copy(const gf_pk_scan* __restrict__ scans, int k,
                                                               const int64_t* __restrict__ start,
                                                               int64_t* __restrict__ block) {
  __shared__ int64_t s_start[GF_PK_ENTRIES(GF_PK_MAX_SCANS) + 1];
  const int n_ent = GF_PK_ENTRIES(k);
  for (int e = threadIdx.x; e <= n_ent; e += GF_SCAN_THREADS) s_start[e] = start[e];
  __syncthreads();
  if (block[2] != 0) return;  // the block is too small: the headers are all there is
  const int64_t pieces = s_start[n_ent] / GF_PK_PIECE;
  uint8_t* __restrict__ out = (uint8_t*)block + GF_PK_HEADER_BYTES(k);
  const int64_t step = (int64_t)gridDim.x * GF_SCAN_THREADS;
  for (int64_t p = (int64_t)blockIdx.x * GF_SCAN_THREADS + threadIdx.x; p < pieces; p += step) {
    const int64_t d0 = p * GF_PK_PIECE;
    int a = 0, b = n_ent;  // s_start[a] <= d0 < s_start[b]
    while (b - a > 1) {
      const int mid = (a + b) >> 1;
      if (s_start[mid] <= d0) a = mid; else b = mid;
    }
    int j = a;
    int c = j / (k + 1), sc = j - c * (k + 1);
    uint4 v = make_uint4(0, 0, 0, 0);
    if (c == GF_PK_SEC_OFFSETS) {
      // (every part of this section is whole int64s and the section starts on the grid: a slot lies in one part)
      int64_t w[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int64_t x = d0 + 8 * h;
        while (x >= s_start[j + 1]) ++j;  // (x < the body's size: ends)
        const int cc = j / (k + 1), ss = j - cc * (k + 1);
        w[h] = 0;
        if (cc == GF_PK_SEC_OFFSETS && ss < k) {
          const int64_t* off = (const int64_t*)scans[ss].d_name_off;
          w[h] = off[(x - s_start[j]) >> 3] - off[0];
        }
      }
      v = make_uint4((uint32_t)w[0], (uint32_t)((uint64_t)w[0] >> 32), (uint32_t)w[1], (uint32_t)((uint64_t)w[1] >> 32));
    } else {
      const uint8_t* src = sc < k ? gf_pk_source(scans, c, sc) + (d0 - s_start[j]) : nullptr;
      if (src && d0 + GF_PK_PIECE <= s_start[j + 1] && ((uintptr_t)src & (GF_PK_PIECE - 1)) == 0) {
        v = *(const uint4*)src;
      } else {
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int d = 0; d < GF_PK_PIECE; ++d) {
          const int64_t x = d0 + d;
          if (x >= s_start[j + 1]) {
            do ++j; while (x >= s_start[j + 1]);  // (x < the body's size: ends)
            // (part j holds byte x, so its scan has what it takes to read it; sections start on the grid, so the
            //  piece stays in its section, and src[d] is the byte for x)
            const int ss = j - c * (k + 1);
            src = ss < k ? gf_pk_source(scans, c, ss) + (d0 - s_start[j]) : nullptr;
          }
          if (src) w[d >> 2] |= (uint32_t)src[d] << (8 * (d & 3));
        }
        v = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
    *(uint4*)(out + d0) = v;
  }
}
