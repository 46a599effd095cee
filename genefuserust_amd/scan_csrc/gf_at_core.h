// The adapter trimming of libgfadapt.so (include/gf_adapter_trim.h), the arithmetic written once: plain C++ that g++
// compiles for the host (tests/cpp/test_adapter_trim_core.cpp, under the sanitizers) and hipcc for the device
// (gf_at_kernels.h).
//
//   the planes of a read   three bit-planes, GF_AT_PLANE words each: the two bits of a base's code ((byte >> 1) & 3:
//                     A 0, C 1, T 2, G 3, either case) and a plane of the bytes that are none of ACGTacgt.  Position i
//                     is bit i & 31 of word 1 + (i >> 5): one zero word in front and three behind a read of
//                     GF_AT_READ_MAX bases, so that a funnel shift at any diagonal stays inside.  The bits outside
//                     [0, L) are zero.  The reverse complement of a read is its planes bit-reversed with the high code
//                     plane flipped (A <-> T, C <-> G is code ^ 2): a[i] and b[I - 1 - i] are complementary exactly when
//                     a and rc(b) hold the same valid code at i and i + L2 - I.
//   a chunk           16 bytes of a read from a 16-byte aligned address, as in gf_pp_core.h: chunk c holds the positions
//                     16 c - a .. 16 c - a + 15.  gf_at_pack_chunk turns it into 16 bits per plane and ORs them in
//                     where they belong; on the device a chunk a lane, with LDS atomics.
//   an insert         one candidate I of the pair overlap: the planes of rc(b) funnel-shifted by L2 - I against those
//                     of a, 32 positions a step: XOR the code planes, OR in the invalid planes, mask to [lo, hi),
//                     popcount.  The walk stops once the differences pass max_diff: they only grow.
//   a round           G candidates, on the device a lane each, the highest I (the lowest p of the sequence step) first:
//                     the first round with an accepted candidate holds the answer.  gf_at_decide_pair below is the
//                     kernel's walk by one thread, lane after lane, over the same functions.
//
// Nothing outside the chunks 0 .. (a + L - 1) / 16 of a read is loaded, and a read of length 0 loads nothing.
#pragma once

#include <stdint.h>

#include "../../include/gf_adapter_trim.h"
#include "gf_pp_core.h"

#define GF_AT_HD GF_PP_HD

#define GF_AT_PLANE 20                     // words of one plane: 1 + GF_AT_READ_MAX / 32 + 3
#define GF_AT_READ_WORDS (3 * GF_AT_PLANE)  // code low, code high, invalid

// the planes of an adapter: bases 0 .. 63, bit j & 31 of word j >> 5 (an adapter is ACGT only: no invalid plane)
struct gf_at_adapter {
  uint32_t lo[2], hi[2];
  int32_t len;
};

GF_AT_HD inline bool gf_at_is_acgt(uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

// NULL, or what is wrong with the settings (include/gf_adapter_trim.h); `single`: the input has no mates
GF_AT_HD inline const char* gf_at_settings_error(const gf_at_settings& s, bool single) {
  if (s.overlap != 0 && s.overlap != 1) return "overlap neither 0 nor 1";
  if (s.min_overlap < 8 || s.min_overlap > GF_AT_READ_MAX) return "min_overlap outside 8 .. 512";
  if (s.max_diff < 0) return "a negative max_diff";
  if (s.diff_percent < 0 || s.diff_percent > 100) return "diff_percent outside 0 .. 100";
  if (s.min_adapter < 4 || s.min_adapter > GF_AT_ADAPTER_MAX) return "min_adapter outside 4 .. 64";
  const int32_t len[2] = {s.adapter_r1_len, s.adapter_r2_len};
  for (int side = 0; side < 2; ++side) {
    if (len[side] == 0) continue;
    if (len[side] < s.min_adapter || len[side] > GF_AT_ADAPTER_MAX)
      return side ? "adapter_r2_len neither 0 nor within min_adapter .. 64"
                  : "adapter_r1_len neither 0 nor within min_adapter .. 64";
    for (int32_t j = 0; j < len[side]; ++j)
      if (!gf_at_is_acgt(side ? s.adapter_r2[j] : s.adapter_r1[j]))
        return side ? "adapter_r2 holds a byte that is not one of ACGT" : "adapter_r1 holds a byte that is not one of ACGT";
  }
  if (s.overlap == 0 && s.adapter_r1_len == 0 && s.adapter_r2_len == 0) return "overlap = 0 with no adapter: nothing to do";
  if (single && s.adapter_r1_len == 0) return "single-end input without adapter_r1";
  return nullptr;
}

GF_AT_HD inline gf_at_adapter gf_at_adapter_planes(const uint8_t* seq, int32_t len) {
  gf_at_adapter ad = {{0, 0}, {0, 0}, len};
  for (int32_t j = 0; j < len && j < GF_AT_ADAPTER_MAX; ++j) {
    ad.lo[j >> 5] |= (uint32_t)((seq[j] >> 1) & 1u) << (j & 31);
    ad.hi[j >> 5] |= (uint32_t)((seq[j] >> 2) & 1u) << (j & 31);
  }
  return ad;
}

// ---- bits ------------------------------------------------------------------------------------------------------------

// bit k of each of a word's four bytes, as four bits (the products of the four single bits never meet)
GF_AT_HD inline uint32_t gf_at_byte_bits(uint32_t w, int k) { return (((w >> k) & 0x01010101u) * 0x10204080u) >> 28; }

GF_AT_HD inline uint32_t gf_at_chunk_bits(const gf_pp_chunk& c, int k) {
  return gf_at_byte_bits(c.w[0], k) | gf_at_byte_bits(c.w[1], k) << 4 | gf_at_byte_bits(c.w[2], k) << 8 |
         gf_at_byte_bits(c.w[3], k) << 12;
}

// 16 bits in reverse order
GF_AT_HD inline uint32_t gf_at_reverse16(uint32_t m) {
  m = ((m & 0x5555u) << 1) | ((m >> 1) & 0x5555u);
  m = ((m & 0x3333u) << 2) | ((m >> 2) & 0x3333u);
  m = ((m & 0x0F0Fu) << 4) | ((m >> 4) & 0x0F0Fu);
  return ((m & 0x00FFu) << 8) | ((m >> 8) & 0x00FFu);
}

// the 32 bits from bit r (0 .. 31) of the 64 bits `high`:`low`
GF_AT_HD inline uint32_t gf_at_funnel(uint32_t low, uint32_t high, int r) {
  return (uint32_t)(((((uint64_t)high) << 32) | low) >> r);
}

// the bits k of a word whose first position is p0 with lo <= p0 + k < hi
GF_AT_HD inline uint32_t gf_at_range(int32_t p0, int32_t lo, int32_t hi) {
  int32_t a = lo - p0, b = hi - p0;
  a = a < 0 ? 0 : a;
  b = b > 32 ? 32 : b;
  if (a >= b) return 0u;
  return (b == 32 ? 0xFFFFFFFFu : (1u << b) - 1u) & ~((1u << a) - 1u);
}

// ---- packing ---------------------------------------------------------------------------------------------------------

// The chunk whose first byte is position p0 (-15 ..) of a read of L bases into the read's planes; rc: into the planes
// of its reverse complement.  or_into(plane, word, bits): planes 0 low, 1 high, 2 invalid; word as in the planes' layout
// (1 + position / 32).
template <class Or>
GF_AT_HD inline void gf_at_pack_chunk(const gf_pp_chunk& ch, int32_t p0, int32_t L, bool rc, Or or_into) {
  uint32_t in = gf_pp_range(p0, 0, L);
  uint32_t bits[3] = {gf_at_chunk_bits(ch, 1) & in, gf_at_chunk_bits(ch, 2) & in, gf_pp_n_mask(ch) & in};
  int32_t at = p0;
  if (rc) {  // byte k is position L - 1 - (p0 + k) of the reverse complement, with the other base of its pair
    in = gf_at_reverse16(in);
    bits[0] = gf_at_reverse16(bits[0]);
    bits[1] = gf_at_reverse16(bits[1]) ^ in;
    bits[2] = gf_at_reverse16(bits[2]);
    at = L - 16 - p0;
  }
  for (int plane = 0; plane < 3; ++plane) {
    uint64_t v = bits[plane];
    int32_t pos = at;
    if (pos < 0) {  // (the bits in front of position 0 are outside the read: zero already)
      v >>= -pos;
      pos = 0;
    }
    v <<= pos & 31;
    if ((uint32_t)v) or_into(plane, 1 + (pos >> 5), (uint32_t)v);
    if (v >> 32) or_into(plane, 2 + (pos >> 5), (uint32_t)(v >> 32));
  }
}

// ---- the pair overlap ------------------------------------------------------------------------------------------------

GF_AT_HD inline bool gf_at_accepted(int32_t ov, int32_t d, const gf_at_settings& s) {
  return ov >= s.min_overlap && d <= s.max_diff && 100 * d <= s.diff_percent * ov;
}

// Whether the insert I is accepted.  A: the planes of a, R: those of rc(b).
GF_AT_HD inline bool gf_at_try_insert(const uint32_t* A, const uint32_t* R, int32_t L1, int32_t L2, int32_t I,
                                      const gf_at_settings& s) {
  const int32_t shift = L2 - I;  // a[i] meets rc(b)[i + shift]
  const int32_t lo = I > L2 ? I - L2 : 0, hi = I < L1 ? I : L1;
  if (hi - lo < s.min_overlap) return false;
  int32_t d = 0;
  for (int32_t w = lo >> 5; w <= (hi - 1) >> 5; ++w) {
    const int32_t t = 32 * w + shift + 32;  // (>= 1: the word holds a position of [lo, hi))
    const int q = t >> 5, r = t & 31;       // rc(b)'s position 32 w + shift is bit r of word q
    const uint32_t diff = (A[w + 1] ^ gf_at_funnel(R[q], R[q + 1], r)) |
                          (A[GF_AT_PLANE + w + 1] ^ gf_at_funnel(R[GF_AT_PLANE + q], R[GF_AT_PLANE + q + 1], r)) |
                          A[2 * GF_AT_PLANE + w + 1] |
                          gf_at_funnel(R[2 * GF_AT_PLANE + q], R[2 * GF_AT_PLANE + q + 1], r);
    d += gf_pp_popcount(diff & gf_at_range(32 * w, lo, hi));
    if (d > s.max_diff) return false;
  }
  return gf_at_accepted(hi - lo, d, s);
}

// the first and the last candidate of a pair; none when first > last
GF_AT_HD inline int32_t gf_at_first_insert(const gf_at_settings& s) { return s.min_overlap; }
GF_AT_HD inline int32_t gf_at_last_insert(int32_t L1, int32_t L2, const gf_at_settings& s) {
  return L1 + L2 - s.min_overlap;
}

// ---- the adapter sequence --------------------------------------------------------------------------------------------

// Whether the adapter lies at position p of the read of L bases with the planes X, 0 <= p <= L - min_adapter.
GF_AT_HD inline bool gf_at_adapter_at(const uint32_t* X, int32_t L, int32_t p, const gf_at_adapter& ad) {
  const int32_t n = ad.len < L - p ? ad.len : L - p;
  const int q = 1 + (p >> 5), r = p & 31;
  int32_t d = 0;
  for (int k = 0; k < 2; ++k) {
    if (32 * k >= n) break;
    const uint32_t diff = (gf_at_funnel(X[q + k], X[q + k + 1], r) ^ ad.lo[k]) |
                          (gf_at_funnel(X[GF_AT_PLANE + q + k], X[GF_AT_PLANE + q + k + 1], r) ^ ad.hi[k]) |
                          gf_at_funnel(X[2 * GF_AT_PLANE + q + k], X[2 * GF_AT_PLANE + q + k + 1], r);
    d += gf_pp_popcount(diff & gf_at_range(32 * k, 0, n));
  }
  return d <= n / 10;
}

// ---- the outcome -----------------------------------------------------------------------------------------------------

// a read untouched by the limits: of length 0, or longer than GF_AT_READ_MAX
GF_AT_HD inline bool gf_at_passes(int64_t len) { return len <= 0 || len > GF_AT_READ_MAX; }

// a mate of L bases of a pair with the insert I*: what it keeps and how
GF_AT_HD inline int gf_at_by_overlap(int32_t L, int32_t insert, int32_t* kept) {
  *kept = insert < L ? insert : L;
  return insert < L ? GF_AT_BY_OVERLAP : GF_AT_OVERLAP_CLEAN;
}

// ---- a pair, by one thread: the walk of gf_at_k_decide, lane after lane ------------------------------------------------

// the planes of a read (or of its reverse complement) from its chunks: load(c), 0 <= c <= (a + L - 1) / 16
template <class Load>
GF_AT_HD inline void gf_at_pack_read(Load load, int a, int32_t L, bool rc, uint32_t* planes) {
  for (int k = 0; k < GF_AT_READ_WORDS; ++k) planes[k] = 0;
  if (L <= 0) return;
  for (int c = 0; c <= (a + L - 1) >> 4; ++c)
    gf_at_pack_chunk(load(c), 16 * c - a, L, rc,
                     [&](int plane, int word, uint32_t bits) { planes[plane * GF_AT_PLANE + word] |= bits; });
}

// I* of a pair, -1 without one: rounds of G candidates from the last downwards
template <int G>
GF_AT_HD inline int32_t gf_at_find_insert(const uint32_t* A, const uint32_t* R, int32_t L1, int32_t L2,
                                          const gf_at_settings& s) {
  for (int32_t top = gf_at_last_insert(L1, L2, s); top >= gf_at_first_insert(s); top -= G) {
    int32_t best = -1;
    for (int gl = 0; gl < G; ++gl) {
      const int32_t I = top - gl;
      if (I >= gf_at_first_insert(s) && I > best && gf_at_try_insert(A, R, L1, L2, I, s)) best = I;
    }
    if (best >= 0) return best;
  }
  return -1;
}

// the smallest p at which the adapter lies in a read, -1 without one: rounds of G positions from 0 upwards
template <int G>
GF_AT_HD inline int32_t gf_at_find_adapter(const uint32_t* X, int32_t L, const gf_at_adapter& ad, int32_t min_adapter) {
  if (ad.len <= 0) return -1;
  for (int32_t p0 = 0; p0 <= L - min_adapter; p0 += G)
    for (int gl = 0; gl < G; ++gl)
      if (p0 + gl <= L - min_adapter && gf_at_adapter_at(X, L, p0 + gl, ad)) return p0 + gl;
  return -1;
}

// One record: a pair (sides 2) or a single-end read (sides 1).  load_l(c) / load_r(c): chunk c of the mates' bases;
// al / ar: how far into its chunk 0 each mate's first byte lies.  kept[side], how[side]: the outcome.
template <int G, class LoadL, class LoadR>
GF_AT_HD inline void gf_at_decide_pair(LoadL load_l, int al, int64_t len_l, LoadR load_r, int ar, int64_t len_r,
                                       int sides, const gf_at_settings& s, int64_t* kept, int* how) {
  kept[0] = len_l;
  kept[1] = len_r;
  how[0] = how[1] = GF_AT_UNTOUCHED;
  if (gf_at_passes(len_l) || (sides == 2 && gf_at_passes(len_r))) return;
  const int32_t L1 = (int32_t)len_l, L2 = sides == 2 ? (int32_t)len_r : 0;
  const gf_at_adapter ad[2] = {gf_at_adapter_planes(s.adapter_r1, s.adapter_r1_len),
                               gf_at_adapter_planes(s.adapter_r2, s.adapter_r2_len)};
  uint32_t A[GF_AT_READ_WORDS], R[GF_AT_READ_WORDS];
  gf_at_pack_read(load_l, al, L1, false, A);
  if (sides == 2 && s.overlap) {
    gf_at_pack_read(load_r, ar, L2, true, R);
    const int32_t insert = gf_at_find_insert<G>(A, R, L1, L2, s);
    if (insert >= 0) {
      int32_t k;
      how[0] = gf_at_by_overlap(L1, insert, &k);
      kept[0] = k;
      how[1] = gf_at_by_overlap(L2, insert, &k);
      kept[1] = k;
      return;
    }
  }
  for (int side = 0; side < sides; ++side) {
    if (ad[side].len <= 0) continue;
    if (side == 1) gf_at_pack_read(load_r, ar, L2, false, R);
    const int32_t p = gf_at_find_adapter<G>(side ? R : A, side ? L2 : L1, ad[side], s.min_adapter);
    if (p >= 0) {
      kept[side] = p;
      how[side] = GF_AT_BY_SEQUENCE;
    }
  }
}
