// The read filter of libgfprep.so (include/gf_read_filter.h), the arithmetic written once: plain C++ that g++ compiles
// for the host (tests/cpp/test_read_filter_core.cpp, under the sanitizers) and hipcc for the device (gf_pp_kernels.h).
//
//   a chunk           16 bytes of a read's bases or qualities as four little-endian words, loaded from a 16-byte aligned
//                     address: with the read's first byte `a` bytes into its chunk 0, chunk c holds the positions
//                     16 c - a .. 16 c - a + 15.  A predicate over a chunk is a mask of 16 bits, bit k for byte k,
//                     computed on the words four bytes at a time; gf_pp_range says which of them lie in [lo, hi).
//   a tile            G consecutive chunks, the last of them the chunk of the read's last byte in round 0; every step
//                     walks the read in tiles from its end towards its start.  On the device a tile is a round of G
//                     lanes, a chunk each (gf_pp_kernels.h); gf_pp_decide_read below is the same walk by one thread,
//                     lane after lane, over the same functions.
//   the window step   S[j] is the sum of the phred values of the tile's first j bytes, j = 0 .. 16 G.  The end
//                     e = p0 + j (p0 the position of the tile's first byte) is looked at in a tile when j >= W, where
//                     the window's sum is S[j] - S[j - W]; the tiles of this step overlap by GF_PP_HALO chunks (80 bytes
//                     >= W + 16), so that every end is looked at in some tile, the higher ends first.
//
// Nothing outside the chunks 0 .. (a + L - 1) / 16 of a read is loaded, and a read of length 0 loads nothing.
#pragma once

#include <stdint.h>

#include "../../include/gf_read_filter.h"

#if defined(__HIPCC__)
#define GF_PP_HD __host__ __device__
#else
#define GF_PP_HD
#endif

#define GF_PP_HALO 5  // chunks two tiles of the window step share: 16 GF_PP_HALO >= GF_PP_WINDOW_MAX + 16

// NULL, or what is wrong with the settings (include/gf_read_filter.h)
GF_PP_HD inline const char* gf_pp_settings_error(const gf_pp_settings& s) {
  if (s.poly_g_min < 0 || s.cut_tail_window < 0 || s.cut_tail_mean < 0 || s.length_required < 0 || s.n_base_limit < 0 ||
      s.qualified_phred < 0 || s.unqualified_percent < 0)
    return "a negative setting";
  if (s.cut_tail_window > GF_PP_WINDOW_MAX) return "cut_tail_window above 64";
  if (s.cut_tail_mean > GF_PP_PHRED_MAX) return "cut_tail_mean above 93";
  if (s.qualified_phred > GF_PP_PHRED_MAX) return "qualified_phred above 93";
  if (s.unqualified_percent > 100) return "unqualified_percent above 100";
  if (s.poly_g_min > GF_MAX_READ_LEN) return "poly_g_min above GF_MAX_READ_LEN";
  if (s.length_required > GF_MAX_READ_LEN) return "length_required above GF_MAX_READ_LEN";
  return nullptr;
}

// ---- four bytes at a time --------------------------------------------------------------------------------------------

// 0x80 in every byte of v that is not 0
GF_PP_HD inline uint32_t gf_pp_nonzero_bytes(uint32_t v) {
  return (((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v) & 0x80808080u;
}

// the 0x80 flags of four bytes as four bits
GF_PP_HD inline uint32_t gf_pp_flag_bits(uint32_t f) {
  f >>= 7;
  return (f | (f >> 7) | (f >> 14) | (f >> 21)) & 0xFu;
}

// bytes that are neither G nor g
GF_PP_HD inline uint32_t gf_pp_word_not_g(uint32_t w) { return gf_pp_nonzero_bytes((w | 0x20202020u) ^ 0x67676767u); }

// bytes that are none of ACGTacgt: | 0x20 folds the cases (only 0x41 and 0x61 give 0x61, and so on), | 0x02 folds a and c
GF_PP_HD inline uint32_t gf_pp_word_n(uint32_t w) {
  const uint32_t x = w | 0x20202020u;
  return gf_pp_nonzero_bytes((x | 0x02020202u) ^ 0x63636363u) & gf_pp_nonzero_bytes(x ^ 0x67676767u) &
         gf_pp_nonzero_bytes(x ^ 0x74747474u);
}

// bytes q < t, for 0 < t <= 127: with 0x80 set in every byte no borrow leaves a byte, and bit 7 of a difference says
// (q & 0x7F) >= t
GF_PP_HD inline uint32_t gf_pp_word_below(uint32_t w, uint32_t t) {
  const uint32_t d = (w | 0x80808080u) - t * 0x01010101u;
  return ~d & ~w & 0x80808080u;
}

// ---- a chunk ---------------------------------------------------------------------------------------------------------

struct gf_pp_chunk {
  uint32_t w[4];
};

GF_PP_HD inline uint32_t gf_pp_not_g_mask(const gf_pp_chunk& c) {
  return gf_pp_flag_bits(gf_pp_word_not_g(c.w[0])) | gf_pp_flag_bits(gf_pp_word_not_g(c.w[1])) << 4 |
         gf_pp_flag_bits(gf_pp_word_not_g(c.w[2])) << 8 | gf_pp_flag_bits(gf_pp_word_not_g(c.w[3])) << 12;
}

GF_PP_HD inline uint32_t gf_pp_n_mask(const gf_pp_chunk& c) {
  return gf_pp_flag_bits(gf_pp_word_n(c.w[0])) | gf_pp_flag_bits(gf_pp_word_n(c.w[1])) << 4 |
         gf_pp_flag_bits(gf_pp_word_n(c.w[2])) << 8 | gf_pp_flag_bits(gf_pp_word_n(c.w[3])) << 12;
}

// the low bases: phred < qualified, that is q < qualified + 33 (none when qualified is 0)
GF_PP_HD inline uint32_t gf_pp_low_mask(const gf_pp_chunk& c, int32_t qualified) {
  if (qualified <= 0) return 0;
  const uint32_t t = (uint32_t)qualified + 33u;
  return gf_pp_flag_bits(gf_pp_word_below(c.w[0], t)) | gf_pp_flag_bits(gf_pp_word_below(c.w[1], t)) << 4 |
         gf_pp_flag_bits(gf_pp_word_below(c.w[2], t)) << 8 | gf_pp_flag_bits(gf_pp_word_below(c.w[3], t)) << 12;
}

GF_PP_HD inline uint32_t gf_pp_phred(uint32_t q) { return q > 33u ? q - 33u : 0u; }

// p[k]: the sum of the phred values of bytes 0 .. k
GF_PP_HD inline void gf_pp_phred_prefix(const gf_pp_chunk& c, uint32_t (&p)[16]) {
  uint32_t sum = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    sum += gf_pp_phred((c.w[k >> 2] >> (8 * (k & 3))) & 0xFFu);
    p[k] = sum;
  }
}

// the bits k of a chunk whose first byte is position p0 with lo <= p0 + k < hi
GF_PP_HD inline uint32_t gf_pp_range(int32_t p0, int32_t lo, int32_t hi) {
  int32_t a = lo - p0, b = hi - p0;
  a = a < 0 ? 0 : a;
  b = b > 16 ? 16 : b;
  return a >= b ? 0u : ((1u << b) - 1u) & ~((1u << a) - 1u);
}

GF_PP_HD inline int gf_pp_top_bit(uint32_t m) { return 31 - __builtin_clz(m); }  // m != 0

GF_PP_HD inline int gf_pp_popcount(uint32_t m) { return __builtin_popcount(m); }

// The ends of chunk i of a tile that close a qualifying window: bit k for the end j = 16 i + k + 1 behind byte k.
// `base` is S[16 i], p the chunk's prefix (so S[j] = base + p[k]), S(j) any earlier S of the tile, `ends` the bits
// whose end e = p0 + j lies in W .. e1.  The sums are compared modulo 2^16, which is how the device keeps S: a window of
// W <= 64 bytes sums to 64 * 222 at the most.
template <class Prefix>
GF_PP_HD inline uint32_t gf_pp_window_ends(int i, uint32_t base, const uint32_t (&p)[16], uint32_t ends, int32_t W,
                                           uint32_t need, Prefix S) {
  uint32_t hit = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int j = 16 * i + k + 1;
    if (j >= W && ((ends >> k) & 1u)) {
      const uint32_t sum = (base + p[k] - S(j - W)) & 0xFFFFu;
      hit |= (uint32_t)(sum >= need) << k;
    }
  }
  return hit;
}

// ---- the verdict -----------------------------------------------------------------------------------------------------

GF_PP_HD inline int gf_pp_reason(int32_t e2, int32_t n_bases, int32_t low, const gf_pp_settings& s) {
  if (e2 < s.length_required) return GF_PP_TOO_SHORT;
  if (n_bases > s.n_base_limit) return GF_PP_TOO_MANY_N;
  if (100 * low > s.unqualified_percent * e2) return GF_PP_LOW_QUALITY;
  return GF_PP_KEPT;
}

// a record's reasons after the pair rule: a mate without a reason of its own is dropped for the other's
GF_PP_HD inline void gf_pp_pair_rule(int& l_reason, int& r_reason) {
  if (l_reason != GF_PP_KEPT && r_reason == GF_PP_KEPT) r_reason = GF_PP_MATE_FAILED;
  else if (r_reason != GF_PP_KEPT && l_reason == GF_PP_KEPT) l_reason = GF_PP_MATE_FAILED;
}

// ---- a read, by one thread: the walk of gf_pp_k_decide, lane after lane -----------------------------------------------

// bases(c) / quals(c): chunk c of the read's bases / qualities, 0 <= c <= (a + L - 1) / 16; ab / aq: how far into its
// chunk 0 the read's first byte lies.  Returns the read's own reason, *e2 its kept length (before the pair rule).
template <int G, class LoadB, class LoadQ>
GF_PP_HD inline int gf_pp_decide_read(LoadB bases, int ab, LoadQ quals, int aq, int32_t L, const gf_pp_settings& s,
                                      int32_t* e2_out) {
  if (L > GF_MAX_READ_LEN) {
    *e2_out = L;
    return GF_PP_KEPT;
  }
  int32_t e1 = L;
  if (s.poly_g_min > 0 && L > 0) {
    int32_t last = -1;  // the last base that is not G
    for (int top = (ab + L - 1) >> 4; last < 0; top -= G) {
      for (int i = G - 1; i >= 0 && last < 0; --i) {
        const int c = top - (G - 1) + i;
        if (c < 0) break;
        const uint32_t m = gf_pp_not_g_mask(bases(c)) & gf_pp_range(16 * c - ab, 0, L);
        if (m) last = 16 * c - ab + gf_pp_top_bit(m);
      }
      if (top - (G - 1) <= 0) break;
    }
    if (L - 1 - last >= s.poly_g_min) e1 = last + 1;
  }
  int32_t e2 = e1;
  const int32_t W = s.cut_tail_window;
  if (W > 0) {
    e2 = 0;
    if (e1 >= W && L > 0) {
      const uint32_t need = (uint32_t)(W * s.cut_tail_mean);
      uint32_t S[16 * G + 1];
      for (int top = (aq + L - 1) >> 4; e2 == 0; top -= G - GF_PP_HALO) {
        const int c0 = top - (G - 1);
        const int32_t p0 = 16 * c0 - aq;
        uint32_t pre[G][16];
        S[0] = 0;
        for (int i = 0; i < G; ++i) {
          gf_pp_chunk ch = {{0, 0, 0, 0}};
          if (c0 + i >= 0) ch = quals(c0 + i);
          gf_pp_phred_prefix(ch, pre[i]);
          for (int k = 0; k < 16; ++k) S[16 * i + k + 1] = (S[16 * i] + pre[i][k]) & 0xFFFFu;
        }
        for (int i = G - 1; i >= 0 && e2 == 0; --i) {
          // the ends behind bytes p0 + 16 i + k: e = that + 1 in W .. e1
          const uint32_t ends = gf_pp_range(p0 + 16 * i + 1, W, e1 + 1);
          const uint32_t hit = gf_pp_window_ends(i, S[16 * i], pre[i], ends, W, need, [&](int j) { return S[j]; });
          if (hit) e2 = p0 + 16 * i + gf_pp_top_bit(hit) + 1;
        }
        if (p0 <= 0) break;
      }
    }
  }
  int32_t n_bases = 0, low = 0;
  if (e2 > 0) {
    for (int c = (ab + L - 1) >> 4; c >= 0; --c) n_bases += gf_pp_popcount(gf_pp_n_mask(bases(c)) & gf_pp_range(16 * c - ab, 0, e2));
    for (int c = (aq + L - 1) >> 4; c >= 0; --c)
      low += gf_pp_popcount(gf_pp_low_mask(quals(c), s.qualified_phred) & gf_pp_range(16 * c - aq, 0, e2));
  }
  *e2_out = e2;
  return gf_pp_reason(e2, n_bases, low, s);
}
