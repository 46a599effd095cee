// The UMI calls of libgfumi.so (include/gf_umi.h), every formula that can go wrong by one written once: plain C++ that
// g++ compiles for the host (tests/cpp/test_umi_core.cpp, under the sanitizers) and hipcc for the device
// (gf_um_kernels.h).  H, mix, fold, the chunks and the pieces are those of gf_dd_core.h.
//
//   a UMI, a field   up to 64 bytes at any alignment: pieces 0 .. 3 of a "record" of that length, hashed as gf_dd_core.h
//                    hashes a record; the same pieces say whether an 'N' is among the bytes and, for a name's field,
//                    whether every byte is one the field may hold.
//   a name line      walked in rounds of G chunks from the chunk of its first byte: per chunk a 16-bit mask of the
//                    spaces and tabs and one of the colons, both cut to the line (gf_um_range).  The token ends at the
//                    lowest set bit of the first; the field starts behind the highest colon in front of that end.  On
//                    the device a lane takes a chunk and ballots answer both (gf_um_kernels.h); gf_um_name_code_host
//                    below is the same walk by one thread, chunk after chunk, over the same functions.
//
// Nothing outside the chunks of a UMI's, a field's or a line's own bytes is loaded; the host walks load no byte outside
// the bounds they are given, the kernels whole chunks (the over-read rule of gf_umi.h).
#pragma once

#include <stdint.h>

#include "../../include/gf_umi.h"
#include "gf_dd_core.h"

#define GF_UM_HD GF_DD_HD

GF_UM_HD inline bool gf_um_inline_source(int32_t source) {
  return source == GF_UM_READ1 || source == GF_UM_READ2 || source == GF_UM_PER_READ;
}

// what gf_umi.h accepts as settings
GF_UM_HD inline bool gf_um_settings_ok(int32_t source, int32_t length, int32_t skip) {
  if (source == GF_UM_NAME) return length == 0 && skip == 0;
  return gf_um_inline_source(source) && length >= 1 && length <= GF_UM_MAX_LEN && skip >= 0 && skip <= GF_UM_MAX_SKIP;
}

// whether side 0 (left) or 1 (right) takes a UMI; single-end input has side 0 only, and PER_READ is READ1 there
GF_UM_HD inline bool gf_um_takes(int32_t source, int side) {
  return source == GF_UM_PER_READ || source == (side ? GF_UM_READ2 : GF_UM_READ1);
}

GF_UM_HD inline uint64_t gf_um_code(uint64_t h) { return h ? h : 1; }

GF_UM_HD inline uint64_t gf_um_code_pair(uint64_t h1, uint64_t h2) { return gf_um_code(gf_dd_mix(h1 + gf_dd_mix(h2 + 1))); }

// K' of a record with key K and code U
GF_UM_HD inline uint64_t gf_um_mix_key(uint64_t K, uint64_t U) {
  if (K == 0 || U == 0) return K;
  const uint64_t k = gf_dd_mix(K + gf_dd_mix(U + 2));
  return k ? k : 1;
}

// whether one of the eight bytes of w is b
GF_UM_HD inline bool gf_um_has_byte(uint64_t w, uint8_t b) {
  const uint64_t x = w ^ (0x0101010101010101ull * b);
  return ((x - 0x0101010101010101ull) & ~x & 0x8080808080808080ull) != 0;
}

// whether a byte may stand in a name's UMI field: one of "ACGTNacgtn+_"
GF_UM_HD inline bool gf_um_field_byte(uint8_t c) {
  const uint8_t f = c & 0xDF;
  return f == 'A' || f == 'C' || f == 'G' || f == 'T' || f == 'N' || c == '+' || c == '_';
}

// whether the first `count` (0 .. 8) bytes of w may all stand in a field
GF_UM_HD inline bool gf_um_word_valid(uint64_t w, int64_t count) {
  bool ok = true;
  for (int b = 0; b < 8; ++b)
    if (b < count) ok = ok && gf_um_field_byte((uint8_t)(w >> (8 * b)));
  return ok;
}

// what piece k of a UMI or field of L bytes adds: to the hash's sum, and whether it holds an 'N' or 'n', or a byte that
// a field may not hold
GF_UM_HD inline void gf_um_piece(const gf_dd_chunk& c0, const gf_dd_chunk& c1, int a, int64_t L, int64_t k, uint64_t& sum,
                                 bool& has_n, bool& invalid) {
  uint64_t w[2];
  gf_dd_piece_words(c0, c1, a, w[0], w[1]);
  for (int h = 0; h < 2; ++h) {
    const int64_t j = 2 * k + h;
    sum += gf_dd_word_term(w[h], L, j);
    // (a byte at or past L is 0 behind the mask: never 'N')
    has_n = has_n || gf_um_has_byte(gf_dd_fold(w[h]) & gf_dd_byte_mask(L, j), 'N');
    const int64_t left = L - 8 * j;
    invalid = invalid || !gf_um_word_valid(w[h], left < 0 ? 0 : left > 8 ? 8 : left);
  }
}

// ---- the inline cut

// whether a taking side's record of L bases is long enough for a UMI of length + skip = c
GF_UM_HD inline bool gf_um_long_enough(int64_t L, int32_t c) { return L >= c; }

// ---- the name line

// the bits of a chunk's 16 bytes, the first of them at position p0, whose positions lie in [lo, hi)
GF_UM_HD inline uint32_t gf_um_range(int64_t p0, int64_t lo, int64_t hi) {
  int64_t a = lo - p0, b = hi - p0;
  a = a < 0 ? 0 : a;
  b = b > 16 ? 16 : b;
  return a >= b ? 0u : ((1u << b) - 1u) & ~((1u << a) - 1u);
}

// bit k: byte k of the chunk is x, or y
GF_UM_HD inline uint32_t gf_um_eq_mask(const gf_dd_chunk& c, uint8_t x, uint8_t y) {
  uint32_t m = 0;
  for (int k = 0; k < 16; ++k) {
    const uint8_t v = (uint8_t)(c.q[k >> 3] >> (8 * (k & 7)));
    m |= (uint32_t)(v == x || v == y) << k;
  }
  return m;
}

GF_UM_HD inline uint32_t gf_um_space_mask(const gf_dd_chunk& c) { return gf_um_eq_mask(c, ' ', '\t'); }
GF_UM_HD inline uint32_t gf_um_colon_mask(const gf_dd_chunk& c) { return gf_um_eq_mask(c, ':', ':'); }

GF_UM_HD inline int gf_um_low_bit(uint32_t m) { return __builtin_ctz(m); }       // m != 0
GF_UM_HD inline int gf_um_high_bit(uint32_t m) { return 31 - __builtin_clz(m); }  // m != 0

// where line 4 i of a text of text_bytes bytes and `newlines` newlines starts and ends; false: no such line
GF_UM_HD inline bool gf_um_name_line(const int64_t* nl_pos, int64_t newlines, int64_t text_bytes, int64_t i, int64_t& s,
                                     int64_t& e) {
  if (i < 0 || i > newlines / 4) return false;  // (keeps 4 i from overflowing)
  const int64_t line = 4 * i;
  s = line == 0 ? 0 : nl_pos[line - 1] + 1;
  e = line < newlines ? nl_pos[line] : text_bytes;
  if (s > text_bytes) s = text_bytes;
  if (e > text_bytes) e = text_bytes;
  if (e < s) e = s;
  return true;
}

// the field behind the token's last colon (at `colon`, -1: none) of a token that ends at `end`: whether it can be a
// UMI by its place and length, where it starts and how long it is
GF_UM_HD inline bool gf_um_field(int64_t colon, int64_t end, int64_t& start, int64_t& len) {
  start = colon + 1;
  len = end - start;
  return colon >= 0 && len >= 1 && len <= GF_UM_MAX_FIELD;
}

// ---- the walks by one thread: what the kernels do, chunk after chunk.  Loads are bounded: a byte outside [lo, hi) is 0.

inline gf_dd_chunk gf_um_load_host(const uint8_t* base, int64_t c, const uint8_t* lo, const uint8_t* hi) {
  gf_dd_chunk v{{0, 0}};
  for (int k = 0; k < 16; ++k) {
    const uintptr_t p = (uintptr_t)base + 16 * c + k;
    if (p >= (uintptr_t)lo && p < (uintptr_t)hi) v.q[k >> 3] |= (uint64_t) * (const uint8_t*)p << (8 * (k & 7));
  }
  return v;
}

// H of the L (<= 64) bytes at `first`, with whether an N is among them and whether a field may not hold one of them
inline uint64_t gf_um_hash_host(const uint8_t* first, int64_t L, bool& has_n, bool& invalid) {
  uint64_t sum = 0;
  has_n = invalid = false;
  if (L > 0) {
    const int a = (int)((uintptr_t)first & 15);
    const uint8_t* base = first - a;
    for (int64_t k = 0; 16 * k < L; ++k) {
      const gf_dd_chunk c0 = gf_um_load_host(base, k, first, first + L);
      const gf_dd_chunk c1 =
          gf_dd_needs_next(a, L, k) ? gf_um_load_host(base, k + 1, first, first + L) : gf_dd_chunk{{0, 0}};
      gf_um_piece(c0, c1, a, L, k, sum, has_n, invalid);
    }
  }
  return gf_dd_finish(L > 0 ? L : 0, sum);
}

// one record of the inline sources: the lengths of its sides (L[1] unused with sides == 1), where their records start
// (first[side]); gives the bytes each side loses at its head (cut[side]; the whole record when emptied), the code and
// whether a UMI holds an N; false: emptied as too short
inline bool gf_um_cut_host(int32_t source, int32_t length, int32_t skip, int sides, const uint8_t* const* first,
                           const int64_t* L, int64_t* cut, uint64_t& code, bool& has_n) {
  const int32_t c = length + skip;
  bool stays = true;
  for (int side = 0; side < sides; ++side)
    if (gf_um_takes(source, side) && !gf_um_long_enough(L[side], c)) stays = false;
  code = 0;
  has_n = false;
  uint64_t h[2] = {0, 0};
  int taken = 0;
  for (int side = 0; side < sides; ++side) {
    cut[side] = stays ? 0 : L[side];
    if (!stays || !gf_um_takes(source, side)) continue;
    bool n = false, invalid = false;
    h[taken++] = gf_um_hash_host(first[side], length, n, invalid);
    has_n = has_n || n;
    cut[side] = c;
  }
  if (stays) code = taken == 2 ? gf_um_code_pair(h[0], h[1]) : gf_um_code(h[0]);
  return stays;
}

// U of the name line text[s .. e) (the line without its newline), 0 when it holds no UMI
inline uint64_t gf_um_name_code_host(const uint8_t* text, int64_t s, int64_t e, bool& has_n) {
  has_n = false;
  if (e > s && text[e - 1] == '\r') --e;
  const int64_t L = e - s;
  const uint8_t* first = text + s;
  const int a = (int)((uintptr_t)first & 15);
  const uint8_t* base = first - a;
  int64_t end = L, colon = -1;
  for (int64_t c = 0; 16 * c - a < L; ++c) {
    const gf_dd_chunk v = gf_um_load_host(base, c, first, first + L);
    const int64_t p0 = 16 * c - a;
    const uint32_t in_line = gf_um_range(p0, 0, L);
    const uint32_t sp = gf_um_space_mask(v) & in_line;
    if (sp) end = p0 + gf_um_low_bit(sp);
    const uint32_t co = gf_um_colon_mask(v) & gf_um_range(p0, 0, end);
    if (co) colon = p0 + gf_um_high_bit(co);
    if (sp) break;
  }
  int64_t start, len;
  if (!gf_um_field(colon, end, start, len)) return 0;
  bool n, invalid;
  const uint64_t h = gf_um_hash_host(first + start, len, n, invalid);
  if (invalid) return 0;
  has_n = n;
  return gf_um_code(h);
}
