// The names of the hit records of a scan (include/gf_hit_names.h), cut from the FASTQ text in HBM:
//
//   where each record's name line lies, and how long it is    gf_hn_k_lengths (a thread per record)
//   where each name goes: an exclusive scan of the lengths    gf_hn_k_scan (one block, in place on the offsets)
//   the names, back to back, in record order                  gf_hn_k_copy (a wavefront per name)
//
// and the whole FASTQ records of the hit records (include/gf_hit_records.h), the same three steps over S spans per
// record (both mates of a pair, whichever read matched):
//
//   where each span lies, and how long it is                   gf_hn_k_rec_lengths (a thread per span)
//   where each span goes                                       gf_hn_k_rec_scan (one block, in place on the offsets)
//   the spans, back to back, in record order                   gf_hn_k_rec_copy (a wavefront per span)
//
// The number of records is on the device (min(totals[0], hits_cap)), so every grid is sized by hits_cap and strides.
// Deterministic: the one atomic of each gather counts the records without a name line / the spans without a record.
#pragma once

#include "../../include/gf_hit_records.h"
#include "gf_scan_common.h"

// one side's FASTQ text and the newline index gf_fastq_index_device wrote for it
struct GfHnText {
  const uint8_t* text;
  const int64_t* nl_pos;
  int64_t n_bytes, n_newlines;
};

__device__ __forceinline__ int64_t gf_hn_records(const int64_t* __restrict__ scan_totals, int64_t hits_cap) {
  const int64_t n = scan_totals[0];
  return n < 0 ? 0 : (n < hits_cap ? n : hits_cap);
}

// ---- lengths: start[k] = where record k's name line starts in its text, off[k] = its length (scanned in place by
// gf_hn_k_scan).  Line 4 i starts after newline 4 i - 1 and ends at newline 4 i, or with the text.
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_hn_k_lengths(
    const gf_pair_hit* __restrict__ hits, const int64_t* __restrict__ scan_totals, int64_t hits_cap,
    int64_t pair_id_base, GfHnText L, GfHnText R, int64_t* __restrict__ start, int64_t* __restrict__ off,
    unsigned long long* __restrict__ n_missing) {
  const int64_t n = gf_hn_records(scan_totals, hits_cap);
  const int64_t step = (int64_t)gridDim.x * GF_SCAN_THREADS;
  for (int64_t k = (int64_t)blockIdx.x * GF_SCAN_THREADS + threadIdx.x; k < n; k += step) {
    const GfHnText& T = hits[k].source == 2 ? R : L;
    const int64_t i = hits[k].pair_id - pair_id_base;
    int64_t s = 0, len = 0;
    // (i <= n_newlines / 4 keeps 4 i from overflowing on a damaged record)
    if (T.text && i >= 0 && i <= T.n_newlines / 4) {
      const int64_t line = 4 * i;
      s = line == 0 ? 0 : T.nl_pos[line - 1] + 1;
      int64_t e = line < T.n_newlines ? T.nl_pos[line] : T.n_bytes;
      s = s < 0 ? 0 : (s > T.n_bytes ? T.n_bytes : s);  // (an index that is not this text's: stay inside the text)
      e = e < s ? s : (e > T.n_bytes ? T.n_bytes : e);
      len = e - s;
    } else {
      atomicAdd(n_missing, 1ull);
    }
    start[k] = s;
    off[k] = len;
  }
}

// ---- scan: off[0 .. n) from lengths to exclusive offsets, off[n] the total; totals [0] .. [2].  One block, in place
// (gf_scan_totals_block).
__global__ __launch_bounds__(GF_SCAN_TOTALS_THREADS) void gf_hn_k_scan(
    const int64_t* __restrict__ scan_totals, int64_t hits_cap, int64_t names_cap, int64_t* __restrict__ off,
    int64_t* __restrict__ totals) {
  const int64_t n = gf_hn_records(scan_totals, hits_cap);
  const long long total = gf_scan_totals_block(off, off, n);
  if (threadIdx.x == 0) {
    off[n] = total;
    totals[0] = n;
    totals[1] = total;
    totals[2] = total > names_cap ? 1 : 0;  // ([3] was counted by gf_hn_k_lengths)
  }
}

// ---- copy: name k by the 64 lanes of one wavefront (lane j: bytes j, j + 64, ..): names are tens of bytes and a
// thread that copied its own would be alone in its wavefront with one round trip per byte.  A name that does not fit
// names_cap is not written at all.
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_hn_k_copy(
    const gf_pair_hit* __restrict__ hits, const int64_t* __restrict__ scan_totals, int64_t hits_cap,
    const uint8_t* __restrict__ l_text, const uint8_t* __restrict__ r_text, const int64_t* __restrict__ start,
    const int64_t* __restrict__ off, uint8_t* __restrict__ names, int64_t names_cap) {
  const int64_t n = gf_hn_records(scan_totals, hits_cap);
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (GF_SCAN_THREADS / 64);
  for (int64_t k = (int64_t)blockIdx.x * (GF_SCAN_THREADS / 64) + (threadIdx.x >> 6); k < n; k += waves) {
    const int64_t o = off[k], len = off[k + 1] - o;
    if (len <= 0 || o + len > names_cap) continue;
    const uint8_t* __restrict__ src = (hits[k].source == 2 ? r_text : l_text) + start[k];
#pragma unroll 1
    for (int64_t j = lane; j < len; j += 64) names[o + j] = src[j];
  }
}

// ---- the records: span S k + s is FASTQ record i = pair_id - pair_id_base of side s (0: L, 1: R), lines 4 i .. 4 i + 3
// without the last newline.  start[] / off[] as above, over S n spans; every record takes both sides.
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_hn_k_rec_lengths(
    const gf_pair_hit* __restrict__ hits, const int64_t* __restrict__ scan_totals, int64_t hits_cap,
    int64_t pair_id_base, int sides, GfHnText L, GfHnText R, int64_t* __restrict__ start, int64_t* __restrict__ off,
    unsigned long long* __restrict__ n_missing) {
  const int64_t spans = gf_hn_records(scan_totals, hits_cap) * sides;
  const int64_t step = (int64_t)gridDim.x * GF_SCAN_THREADS;
  for (int64_t j = (int64_t)blockIdx.x * GF_SCAN_THREADS + threadIdx.x; j < spans; j += step) {
    const int64_t k = sides == 2 ? j >> 1 : j;
    const GfHnText& T = (sides == 2 && (j & 1)) ? R : L;
    const int64_t i = hits[k].pair_id - pair_id_base;
    int64_t s = 0, len = 0;
    // (i <= n_newlines / 4 keeps 4 i from overflowing on a damaged record)
    if (T.text && i >= 0 && i <= T.n_newlines / 4) {
      const int64_t line = 4 * i;
      s = line == 0 ? 0 : T.nl_pos[line - 1] + 1;
      int64_t e = line + 3 < T.n_newlines ? T.nl_pos[line + 3] : T.n_bytes;
      s = s < 0 ? 0 : (s > T.n_bytes ? T.n_bytes : s);  // (an index that is not this text's: stay inside the text)
      e = e < s ? s : (e > T.n_bytes ? T.n_bytes : e);
      len = e - s;
    } else {
      atomicAdd(n_missing, 1ull);
    }
    start[j] = s;
    off[j] = len;
  }
}

__global__ __launch_bounds__(GF_SCAN_TOTALS_THREADS) void gf_hn_k_rec_scan(
    const int64_t* __restrict__ scan_totals, int64_t hits_cap, int sides, int64_t records_cap, int64_t* off,
    int64_t* __restrict__ totals) {
  const int64_t spans = gf_hn_records(scan_totals, hits_cap) * sides;
  const long long total = gf_scan_totals_block(off, off, spans);
  if (threadIdx.x == 0) {
    off[spans] = total;
    totals[0] = spans;
    totals[1] = total;
    totals[2] = total > records_cap ? 1 : 0;  // ([3] was counted by gf_hn_k_rec_lengths)
  }
}

// A span is 300 to 1300 bytes (two lines of a read's length and two short ones): 5 to 20 rounds of the wavefront at a
// byte per lane, every round one contiguous 64-byte piece of source and destination.  A span that does not fit
// records_cap is not written at all.
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_hn_k_rec_copy(
    const int64_t* __restrict__ scan_totals, int64_t hits_cap, int sides, const uint8_t* __restrict__ l_text,
    const uint8_t* __restrict__ r_text, const int64_t* __restrict__ start, const int64_t* __restrict__ off,
    uint8_t* __restrict__ records, int64_t records_cap) {
  const int64_t spans = gf_hn_records(scan_totals, hits_cap) * sides;
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (GF_SCAN_THREADS / 64);
  for (int64_t j = (int64_t)blockIdx.x * (GF_SCAN_THREADS / 64) + (threadIdx.x >> 6); j < spans; j += waves) {
    const int64_t o = off[j], len = off[j + 1] - o;
    if (len <= 0 || o + len > records_cap) continue;
    const uint8_t* __restrict__ src = ((sides == 2 && (j & 1)) ? r_text : l_text) + start[j];
#pragma unroll 1
    for (int64_t b = lane; b < len; b += 64) records[o + b] = src[b];
  }
}
