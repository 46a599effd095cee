// The read QC of libgfqc.so (include/gf_read_qc.h), the arithmetic written once: plain C++ that g++ compiles for the
// host (tests/cpp/test_read_qc_core.cpp, under the sanitizers) and hipcc for the device (gf_qc_kernels.h).
//
//   a base            one byte of bases and one of qualities: gf_qc_count adds its eight columns to a row by compares,
//                     never by an index computed from the byte.
//   a lane            the walk of a record is split by cycle mod 64: lane l takes the cycles l, l + 64, .. of every
//                     record.  The cycles below GF_QC_CYCLES are 8 per lane, and their 8 x 8 counts are 32-bit
//                     accumulators that live across records (registers on the device); every later cycle of the lane
//                     goes to the one tail row, in 64-bit.  gf_qc_lane_record is that walk for one lane and one
//                     record, the text gf_qc_k_stats runs; gf_qc_walk_record below is the kernel's walk by one thread,
//                     lane after lane, over the same function.
//   overflow          a record adds at most one base to each of a lane's 8 cycle rows, so a 32-bit accumulator grows by
//                     at most 222 (qual_sum: phred <= 255 - 33) per record.  After GF_QC_FLUSH_RECORDS = 2^20 records
//                     it is at most 222 * 2^20 < 2^28, and is flushed and zeroed then, whatever n is.  The tail row and
//                     the tables are 64-bit: they sum bytes that exist in memory.
//   an insert         a pair's entry of the insert histogram is the overlap walk of gf_at_core.h as it is, with that
//                     predicate's default settings fixed here; gf_qc_pair_entry is gf_qc_k_insert's walk by one thread.
//
// Nothing outside a record's bytes 0 .. L - 1 is asked of the loaders, and a record of length 0 loads nothing.
#pragma once

#include <stdint.h>

#include "../../include/gf_read_qc.h"
#include "gf_at_core.h"
#include "gf_pp_core.h"

#define GF_QC_LANES 64                                  // the lanes that share a record
#define GF_QC_LANE_CYCLES (GF_QC_CYCLES / GF_QC_LANES)  // cycle rows a lane keeps: 8
#define GF_QC_FLUSH_RECORDS (1 << 20)                   // records a lane's 32-bit accumulators may take between flushes

// the entry of length_hist a record of length L (>= 0) counts in
GF_PP_HD inline int gf_qc_length_entry(int64_t L) { return L < GF_QC_CYCLES ? (int)L : GF_QC_CYCLES; }

// the row of cycle[][] the base at position pos (>= 0) counts in
GF_PP_HD inline int gf_qc_row(int64_t pos) { return pos < GF_QC_CYCLES ? (int)pos : GF_QC_CYCLES; }

// the word of a side's table that holds column col of row `row`
GF_PP_HD inline int gf_qc_word(int row, int col) { return GF_QC_CYCLES + 1 + row * GF_QC_COLUMNS + col; }

// a record's length from its offsets: offsets that run backwards give 0
GF_PP_HD inline int64_t gf_qc_length(int64_t start, int64_t end) { return end > start ? end - start : 0; }

// one base with the byte b and the quality byte q, added to its row when valid is 1, nothing when it is 0 (no branch:
// | and &, not || and &&)
template <class T>
GF_PP_HD inline void gf_qc_count(uint32_t b, uint32_t q, T (&row)[GF_QC_COLUMNS], uint32_t valid = 1u) {
  const uint32_t x = b | 0x20u;  // folds the cases: only 0x41 and 0x61 give 0x61, and so on
  const uint32_t is_a = x == 0x61u, is_c = x == 0x63u, is_g = x == 0x67u, is_t = x == 0x74u;
  const uint32_t phred = gf_pp_phred(q);
  row[GF_QC_COL_A] += (T)(is_a & valid);
  row[GF_QC_COL_C] += (T)(is_c & valid);
  row[GF_QC_COL_G] += (T)(is_g & valid);
  row[GF_QC_COL_T] += (T)(is_t & valid);
  row[GF_QC_COL_N] += (T)((1u - (is_a | is_c | is_g | is_t)) & valid);
  row[GF_QC_COL_QUAL_SUM] += (T)(phred & (0u - valid));
  row[GF_QC_COL_Q20] += (T)((uint32_t)(phred >= 20u) & valid);
  row[GF_QC_COL_Q30] += (T)((uint32_t)(phred >= 30u) & valid);
}

// The first K rounds of 64 cycles of a record by lane `lane`, K = the rounds the record has below GF_QC_CYCLES, so only
// round K - 1 may end inside the wavefront: head = min(L, GF_QC_CYCLES) > 64 (K - 1).  All 2 K bytes are loaded before
// the first is counted, in straight-line code, so that on the device the loads of a record are in flight together; a
// lane past the record's end loads the record's last byte again and does not count it.
template <int K, class LoadB, class LoadQ>
GF_PP_HD inline void gf_qc_lane_rounds(LoadB base, LoadQ qual, int head, int lane,
                                       uint32_t (&acc)[GF_QC_LANE_CYCLES][GF_QC_COLUMNS]) {
  uint32_t b[K], q[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int pos = GF_QC_LANES * k + lane;
    const int at = k < K - 1 || pos < head ? pos : head - 1;
    b[k] = base(at);
    q[k] = qual(at);
  }
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (k < K - 1 || GF_QC_LANES * k + lane < head) gf_qc_count(b[k], q[k], acc[k]);
}

// One record of L (>= 0) bases by lane `lane`: base(pos) / qual(pos) give byte pos, 0 <= pos < L.  acc[k]: the lane's
// row of cycle 64 k + lane; tail: its share of row GF_QC_CYCLES.  The number of rounds is the same for every lane of
// the record: on the device a scalar branch.
template <class LoadB, class LoadQ>
GF_PP_HD inline void gf_qc_lane_record(LoadB base, LoadQ qual, int64_t L, int lane,
                                       uint32_t (&acc)[GF_QC_LANE_CYCLES][GF_QC_COLUMNS],
                                       uint64_t (&tail)[GF_QC_COLUMNS]) {
  const int head = L < GF_QC_CYCLES ? (int)L : GF_QC_CYCLES;
  switch ((head + GF_QC_LANES - 1) / GF_QC_LANES) {
    case 1: gf_qc_lane_rounds<1>(base, qual, head, lane, acc); break;
    case 2: gf_qc_lane_rounds<2>(base, qual, head, lane, acc); break;
    case 3: gf_qc_lane_rounds<3>(base, qual, head, lane, acc); break;
    case 4: gf_qc_lane_rounds<4>(base, qual, head, lane, acc); break;
    case 5: gf_qc_lane_rounds<5>(base, qual, head, lane, acc); break;
    case 6: gf_qc_lane_rounds<6>(base, qual, head, lane, acc); break;
    case 7: gf_qc_lane_rounds<7>(base, qual, head, lane, acc); break;
    case 8: gf_qc_lane_rounds<8>(base, qual, head, lane, acc); break;
    default: break;  // (a record of length 0)
  }
  for (int64_t pos = GF_QC_CYCLES + lane; pos < L; pos += GF_QC_LANES) gf_qc_count(base(pos), qual(pos), tail);
}

// a lane's accumulators into a table: add(word, value) for every count that is not 0; the accumulators are zeroed
template <class Add>
GF_PP_HD inline void gf_qc_lane_flush(int lane, uint32_t (&acc)[GF_QC_LANE_CYCLES][GF_QC_COLUMNS],
                                      uint64_t (&tail)[GF_QC_COLUMNS], Add add) {
#pragma unroll
  for (int k = 0; k < GF_QC_LANE_CYCLES; ++k) {
#pragma unroll
    for (int col = 0; col < GF_QC_COLUMNS; ++col) {
      if (acc[k][col]) add(gf_qc_word(GF_QC_LANES * k + lane, col), (uint64_t)acc[k][col]);
      acc[k][col] = 0;
    }
  }
#pragma unroll
  for (int col = 0; col < GF_QC_COLUMNS; ++col) {
    if (tail[col]) add(gf_qc_word(GF_QC_CYCLES, col), tail[col]);
    tail[col] = 0;
  }
}

// ---- a record, by one thread: the walk of gf_qc_k_stats, lane after lane -------------------------------------------

// adds the record to table (int64[GF_QC_SIDE_WORDS]); len: its length as the offsets give it, negative included
template <class LoadB, class LoadQ>
GF_PP_HD inline void gf_qc_walk_record(LoadB base, LoadQ qual, int64_t len, int64_t* table) {
  const int64_t L = len < 0 ? 0 : len;
  table[gf_qc_length_entry(L)] += 1;
  for (int lane = 0; lane < GF_QC_LANES; ++lane) {
    uint32_t acc[GF_QC_LANE_CYCLES][GF_QC_COLUMNS] = {};
    uint64_t tail[GF_QC_COLUMNS] = {};
    gf_qc_lane_record(base, qual, L, lane, acc, tail);
    gf_qc_lane_flush(lane, acc, tail, [&](int word, uint64_t v) { table[word] += (int64_t)v; });
  }
}

// ---- the insert histogram ------------------------------------------------------------------------------------------

// the overlap predicate's settings, fixed here: the defaults of gf_adapter_trim.h, no adapter sequence
GF_PP_HD inline gf_at_settings gf_qc_insert_settings() {
  gf_at_settings s = {};
  s.overlap = 1;
  s.min_overlap = GF_QC_INSERT_MIN;
  s.max_diff = 5;
  s.diff_percent = 20;
  s.min_adapter = 10;
  return s;
}

// whether a mate of this length is measured: 1 .. GF_AT_READ_MAX bases
GF_PP_HD inline bool gf_qc_measured(int64_t len) { return len >= 1 && len <= GF_AT_READ_MAX; }

// the entry of the histogram a measured pair counts in: I*, or 0 without one (insert < 0)
GF_PP_HD inline int gf_qc_insert_entry(int32_t insert) { return insert < 0 ? 0 : (int)insert; }

// A pair, by one thread: the walk of gf_qc_k_insert over gf_at_core.h.  load_l(c) / load_r(c): chunk c of the mates'
// bases; al / ar: how far into its chunk 0 each mate's first byte lies.  Returns the entry the pair counts in.
template <int G, class LoadL, class LoadR>
GF_PP_HD inline int gf_qc_pair_entry(LoadL load_l, int al, int64_t len_l, LoadR load_r, int ar, int64_t len_r) {
  if (!gf_qc_measured(len_l) || !gf_qc_measured(len_r)) return GF_QC_INSERT_UNMEASURED;
  const gf_at_settings s = gf_qc_insert_settings();
  uint32_t A[GF_AT_READ_WORDS], R[GF_AT_READ_WORDS];
  gf_at_pack_read(load_l, al, (int32_t)len_l, false, A);
  gf_at_pack_read(load_r, ar, (int32_t)len_r, true, R);
  return gf_qc_insert_entry(gf_at_find_insert<G>(A, R, (int32_t)len_l, (int32_t)len_r, s));
}
