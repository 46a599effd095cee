// The report tail of libgfreport.so, written once: plain C++ that g++ compiles for the host (tests/cpp/
// test_report_core.cpp, under the sanitizers) and hipcc for the device (gf_rp_kernels.h).  Three things per match:
//
//   the filter reason          FusionMapper::filter_matches without remove_alignables (fusion_mapper.rs:276-376,
//                              :559-569), gf_readmatch_filter's numbers
//   the Levenshtein distance   Hyyro's block bit-vector recurrence, the algorithm of edit_distance.rs:12-92
//   calc_ed and the shift      FusionResult::calc_ed for one shift (fusion_result.rs:326-410) and the choice over the
//                              shifts -3 .. 3 of adjust_fusion_break (:299-324)
//
// On the device one wavefront runs this text with the same values.  What differs between host and device is the
// Wave, the 64 words a wavefront has one of per lane:
//     w.load_pattern(p, n)     word j of the wave's pattern block = p[j] for j < n, else "none"
//     w.load_symbols(p, n)     the same for the wave's chunk of the text
//     w.eq(c)                  the 64-bit mask of the pattern block's symbols that equal c   (device: one ballot)
//     w.symbol(j)              text symbol j, the same value in every lane                       (device: one readlane)
//     w.carry_load / _store    word k of two 64 x 64-bit carry vectors                       (device: readlanes, a masked move)
//     w.unequal_neighbours     how many i in [0, n - 1) have s[i] != s[i + 1]                (device: strided ballots)
//
// The distance runs block-major: the pattern's 64-symbol blocks are the outer loop, the text the inner one.  A block's
// vertical deltas then live in two scalars for its whole pass, and what block r hands to block r + 1 — one horizontal
// carry bit pair per text symbol — is a bit vector over the text, 64 symbols a lane.  Nothing is indexed at run time
// but lanes, there is no array per thread, and the inner loop touches no memory.  The text is the shorter of the two
// strings and has at most GF_RP_MAX_LEN symbols (64 lanes of 64 carry bits); the pattern may have any length.
//
// Every loop is bounded by a length its caller read once; nothing outside [0, length) of either string is read.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define GF_RP_HD __host__ __device__
#else
#define GF_RP_HD
#endif

#define GF_RP_MAX_LEN 4096       // GF_MAX_READ_LEN: symbols of a read, and of the shorter string of a distance
#define GF_RP_SHIFTS 7           // -3 .. 3
#define GF_RP_WINDOW 20          // the bases either side of the break that decide the shift
#define GF_RP_NO_SYMBOL 256u     // a word of the wave past the end of its symbols

// a match's status (gf_rp_adjust_device; include/gf_report.h names them too)
#define GF_RP_OK 0
#define GF_RP_OUT_OF_DOMAIN 1    // a shift puts the break outside (0, len): the caller computes this match on the host
#define GF_RP_BAD_ROW 2          // offsets, cluster or references that point outside their arrays, or a read too long

// negative filter reasons
#define GF_RP_BAD_BREAK (-1)     // read_break + 1 outside [0, len]: the reference's subchars panics
#define GF_RP_BAD_READ (-2)      // offsets outside the bases

// the fields of gf_readmatch (include/gfmatch.h) the filter reads
struct GfRpMatch {
  int32_t read_break, left_distance, right_distance, left_position, right_position, left_contig, right_contig;
};

// ---- the filter --------------------------------------------------------------------------------------------------------

// fusion_mapper.rs:559-569 given dis_connected_count
GF_RP_HD inline bool gf_rp_low_complexity(int64_t n, int64_t unequal) { return n < 20 || unequal < 7; }

template <class Wave>
GF_RP_HD inline int32_t gf_rp_filter_reason(Wave& w, const GfRpMatch& m, const uint8_t* seq, int64_t len,
                                            int32_t deletion_threshold) {
  const int64_t cut = (int64_t)m.read_break + 1;
  if (cut < 0 || cut > len) return GF_RP_BAD_BREAK;
  if (gf_rp_low_complexity(cut, w.unequal_neighbours(seq, cut)) ||
      gf_rp_low_complexity(len - cut, w.unequal_neighbours(seq + cut, len - cut)))
    return 1;
  if (m.left_distance + m.right_distance >= 5) return 2;
  if (m.left_contig == m.right_contig) {
    int64_t d = (int64_t)m.left_position - (int64_t)m.right_position;
    if (d < 0) d = -d;
    if (d < (int64_t)deletion_threshold) return 3;
  }
  return 0;
}

// ---- the distance ------------------------------------------------------------------------------------------------------

// Levenshtein distance of a[0, an) and b[0, bn); -1 when the shorter has more than GF_RP_MAX_LEN symbols.
template <class Wave>
GF_RP_HD inline int32_t gf_rp_edit_distance(Wave& w, const uint8_t* a, int32_t an, const uint8_t* b, int32_t bn) {
  if (an < 0 || bn < 0) return -1;
  // the longer string is the pattern
  const uint8_t* p = an >= bn ? a : b;
  const uint8_t* t = an >= bn ? b : a;
  const int32_t m = an >= bn ? an : bn, n = an >= bn ? bn : an;
  if (n == 0) return m;
  if (n > GF_RP_MAX_LEN) return -1;
  const int32_t tmax = (m - 1) >> 6;       // the last block
  const int32_t chunks = (n + 63) >> 6;    // of 64 text symbols
  const uint64_t msb = 1ull << 63;
  int32_t d = m;
  for (int32_t r = 0; r <= tmax; r++) {
    const int32_t in_block = r == tmax ? m - 64 * tmax : 64;
    w.load_pattern(p + 64 * r, in_block);
    uint64_t vp = in_block == 64 ? ~0ull : ((1ull << in_block) - 1), vn = 0;
    const uint64_t top = 1ull << (in_block - 1);
    for (int32_t k = 0; k < chunks; k++) {
      const int32_t in_chunk = k == chunks - 1 ? n - 64 * k : 64;
      w.load_symbols(t + 64 * k, in_chunk);
      // bit j: what block r - 1 carried out at text symbol 64 k + j (block 0: +1 every step, -1 never)
      uint64_t cp = ~0ull, cn = 0;
      if (r > 0) w.carry_load(k, cp, cn);
      uint64_t op = 0, on = 0;
      for (int32_t j = 0; j < in_chunk; j++) {
        uint64_t x = w.eq(w.symbol(j));
        const bool carry_n = (cn >> j) & 1;
        if (carry_n) x |= 1ull;
        const uint64_t d0 = (((x & vp) + vp) ^ vp) | x | vn;
        const uint64_t hp = vn | ~(d0 | vp);
        const uint64_t hn = d0 & vp;
        uint64_t y = hp << 1;
        if ((cp >> j) & 1) y |= 1ull;
        vp = (hn << 1) | ~(d0 | y);
        if (carry_n) vp |= 1ull;
        vn = d0 & y;
        if (hp & msb) op |= 1ull << j;
        if (hn & msb) on |= 1ull << j;
        if (r == tmax) {
          if (hp & top) d++;
          else if (hn & top) d--;
        }
      }
      if (r < tmax) w.carry_store(k, op, on);
    }
  }
  return d;
}

// ---- calc_ed and the choice of the shift -------------------------------------------------------------------------------

struct GfRpSide {
  int32_t window;   // the distance over the GF_RP_WINDOW symbols next to the break
  int32_t whole;    // the distance over the whole overlap
};

// Whether every shift keeps the break inside the read: 0 < read_break + shift + 1 < len for shift in -3 .. 3.
GF_RP_HD inline bool gf_rp_in_domain(int64_t read_break, int64_t len) { return read_break - 3 + 1 > 0 && read_break + 3 + 1 < len; }

// One side of calc_ed for one shift (fusion_result.rs:326-410).  left: the read's first left_len symbols against the end
// of the cluster's left reference; right: the rest against the start of its right reference.  In the domain only.
template <class Wave>
GF_RP_HD inline GfRpSide gf_rp_calc_ed_side(Wave& w, bool right, const uint8_t* seq, int32_t len, int32_t left_len,
                                            const uint8_t* ref, int32_t ref_len) {
  const int32_t part = right ? len - left_len : left_len;
  const int32_t whole = part < ref_len ? part : ref_len;
  const int32_t window = whole < GF_RP_WINDOW ? whole : GF_RP_WINDOW;
  GfRpSide out;
  if (right) {
    out.window = gf_rp_edit_distance(w, seq + left_len, window, ref, window);
    out.whole = gf_rp_edit_distance(w, seq + left_len, whole, ref, whole);
  } else {
    out.window = gf_rp_edit_distance(w, seq + left_len - window, window, ref + ref_len - window, window);
    out.whole = gf_rp_edit_distance(w, seq + left_len - whole, whole, ref + ref_len - whole, whole);
  }
  return out;
}

struct GfRpAdjust {
  int32_t shift, left_distance, right_distance, status;
};

// adjust_fusion_break's choice: sides[2 * s] / sides[2 * s + 1] = the left / right side of shift s - 3.  The first
// shift, in the order -3 .. 3, whose window total is strictly smallest.
GF_RP_HD inline GfRpAdjust gf_rp_choose_shift(const GfRpSide* sides) {
  GfRpAdjust out = {0, 0, 0, GF_RP_OK};
  int32_t smallest = 0xFFFF;
  for (int32_t s = 0; s < GF_RP_SHIFTS; s++) {
    const int32_t total = sides[2 * s].window + sides[2 * s + 1].window;
    if (total < smallest) {
      smallest = total;
      out.shift = s - 3, out.left_distance = sides[2 * s].whole, out.right_distance = sides[2 * s + 1].whole;
    }
  }
  return out;
}

// ---- the wave on the host ----------------------------------------------------------------------------------------------

#if !defined(__HIP_DEVICE_COMPILE__)
struct GfRpHostWave {
  uint32_t pat[64], sym[64];
  uint64_t cp[64], cn[64];

  void load_pattern(const uint8_t* p, int32_t n) {
    for (int32_t j = 0; j < 64; j++) pat[j] = j < n ? p[j] : GF_RP_NO_SYMBOL;
  }
  void load_symbols(const uint8_t* p, int32_t n) {
    for (int32_t j = 0; j < 64; j++) sym[j] = j < n ? p[j] : GF_RP_NO_SYMBOL;
  }
  uint32_t symbol(int32_t j) const { return sym[j]; }
  uint64_t eq(uint32_t c) const {
    uint64_t x = 0;
    for (int32_t j = 0; j < 64; j++) x |= (uint64_t)(pat[j] == c) << j;
    return x;
  }
  void carry_load(int32_t k, uint64_t& p, uint64_t& n) const { p = cp[k], n = cn[k]; }
  void carry_store(int32_t k, uint64_t p, uint64_t n) { cp[k] = p, cn[k] = n; }
  int64_t unequal_neighbours(const uint8_t* s, int64_t n) const {
    int64_t diff = 0;
    for (int64_t i = 0; i + 1 < n; i++) diff += s[i] != s[i + 1];
    return diff;
  }
};
#endif
