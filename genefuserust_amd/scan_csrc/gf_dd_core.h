// The duplicate removal of libgfdedup.so (include/gf_dedup.h), every formula that can go wrong by one written once:
// plain C++ that g++ compiles for the host (tests/cpp/test_dedup_core.cpp, under the sanitizers) and hipcc for the
// device (gf_dd_kernels.h).
//
//   a chunk      16 bytes of a record's bases as two little-endian 64-bit words, loaded from a 16-byte aligned address:
//                with the record's first byte `a` bytes into its chunk 0, chunk c holds the positions 16 c - a ..
//                16 c - a + 15, and the record's last byte lies in chunk top = (a + L - 1) / 16.
//   a piece      the record's bytes 16 k .. 16 k + 15, its words 2 k and 2 k + 1: what one lane takes.  They lie in the
//                chunks k and k + 1, shifted by `a` bytes (gf_dd_piece_words: a funnel shift over three of the four
//                words).  Chunk k + 1 is needed, and loaded, only with a > 0 and k + 1 <= top: bytes past the top
//                chunk are past L and count as 0 anyway.
//   a round      G consecutive pieces, a lane each (gf_dd_kernels.h); gf_dd_hash_record below is the same walk by one
//                thread, piece after piece, over the same functions.  The sum over the words does not depend on
//                their order.
//
// Nothing outside the chunks 0 .. top of a record is loaded, and a record of length 0 loads nothing.
#pragma once

#include <stdint.h>

#include "../../include/gf_dedup.h"

#if defined(__HIPCC__)
#define GF_DD_HD __host__ __device__
#else
#define GF_DD_HD
#endif

#define GF_DD_GOLDEN 0x9E3779B97F4A7C15ull
#define GF_DD_NO_INDEX 0x7FFFFFFFFFFFFFFFll  // first[] of an empty slot: INT64_MAX

struct gf_dd_chunk {
  uint64_t q[2];
};

// fold of eight bytes at once
GF_DD_HD inline uint64_t gf_dd_fold(uint64_t w) { return w & 0xDFDFDFDFDFDFDFDFull; }

GF_DD_HD inline uint64_t gf_dd_mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// the length of record i of offsets that need neither start at 0 nor run forwards
GF_DD_HD inline int64_t gf_dd_length(int64_t start, int64_t end) { return end > start ? end - start : 0; }

// the bytes of word j that lie in front of L, as a mask; 0 for a word the record does not have (8 j >= L)
GF_DD_HD inline uint64_t gf_dd_byte_mask(int64_t L, int64_t j) {
  const int64_t left = L - 8 * j;
  if (left <= 0) return 0;
  return left >= 8 ? ~0ull : (1ull << (8 * left)) - 1ull;
}

// bytes s .. s + 7 of the 16 bytes lo, hi (s = 0 .. 7)
GF_DD_HD inline uint64_t gf_dd_funnel(uint64_t lo, uint64_t hi, int s) {
  return s == 0 ? lo : (lo >> (8 * s)) | (hi << (64 - 8 * s));
}

// the two words of the piece whose first byte lies `a` bytes (0 .. 15) into chunk c0; c1 is the chunk behind it
GF_DD_HD inline void gf_dd_piece_words(const gf_dd_chunk& c0, const gf_dd_chunk& c1, int a, uint64_t& w0,
                                       uint64_t& w1) {
  if (a < 8) {
    w0 = gf_dd_funnel(c0.q[0], c0.q[1], a);
    w1 = gf_dd_funnel(c0.q[1], c1.q[0], a);
  } else {
    w0 = gf_dd_funnel(c0.q[1], c1.q[0], a - 8);
    w1 = gf_dd_funnel(c1.q[0], c1.q[1], a - 8);
  }
}

// what word j of a record of L bases adds to the sum: nothing when the record has no such word
GF_DD_HD inline uint64_t gf_dd_word_term(uint64_t w, int64_t L, int64_t j) {
  if (8 * j >= L) return 0;
  return gf_dd_mix((gf_dd_fold(w) & gf_dd_byte_mask(L, j)) + (uint64_t)(j + 1) * GF_DD_GOLDEN);
}

// what piece k of a record of L bases adds to the sum
GF_DD_HD inline uint64_t gf_dd_piece_sum(const gf_dd_chunk& c0, const gf_dd_chunk& c1, int a, int64_t L, int64_t k) {
  uint64_t w0, w1;
  gf_dd_piece_words(c0, c1, a, w0, w1);
  return gf_dd_word_term(w0, L, 2 * k) + gf_dd_word_term(w1, L, 2 * k + 1);
}

// whether piece k needs the chunk behind its own
GF_DD_HD inline bool gf_dd_needs_next(int a, int64_t L, int64_t k) { return a > 0 && k + 1 <= (a + L - 1) >> 4; }

// H from the sum over the words; H of no bases is mix(0) = 0
GF_DD_HD inline uint64_t gf_dd_finish(int64_t L, uint64_t sum) { return gf_dd_mix((uint64_t)L + sum); }

GF_DD_HD inline uint64_t gf_dd_key_single(int64_t L, uint64_t h) {
  if (L <= 0) return 0;
  return h ? h : 1;
}

GF_DD_HD inline uint64_t gf_dd_key_pair(int64_t L1, uint64_t h1, int64_t L2, uint64_t h2) {
  if (L1 + L2 <= 0) return 0;
  const uint64_t k = gf_dd_mix(h1 + gf_dd_mix(h2 + 1));
  return k ? k : 1;
}

// the table: a key's home slot, and the slot a probe looks at next (slots a power of two)
GF_DD_HD inline int64_t gf_dd_home(uint64_t key, int64_t slots) { return (int64_t)(key & (uint64_t)(slots - 1)); }
GF_DD_HD inline int64_t gf_dd_next(int64_t s, int64_t slots) { return (s + 1) & (slots - 1); }

GF_DD_HD inline bool gf_dd_slots_ok(int64_t slots) {
  return slots >= GF_DD_MIN_SLOTS && (slots & (slots - 1)) == 0;
}

// the histogram's entry of a key offered c times; 0: none (the slot is empty, or nothing was counted)
GF_DD_HD inline int gf_dd_level(uint32_t c) { return c < GF_DD_LEVELS - 1 ? (int)c : GF_DD_LEVELS - 1; }

// ---- the walks by one thread: what the kernels do, piece after piece and slot after slot ------------------------------

// chunk c behind the 16-byte aligned address p (the host's load; the kernels' is gf_dd_load in gf_dd_kernels.h)
inline gf_dd_chunk gf_dd_load_host(const uint8_t* p, int64_t c) {
  gf_dd_chunk v;
  for (int h = 0; h < 2; ++h) {
    v.q[h] = 0;
    for (int b = 0; b < 8; ++b) v.q[h] |= (uint64_t)p[16 * c + 8 * h + b] << (8 * b);
  }
  return v;
}

// H of the record of L bases at `first`, any alignment
inline uint64_t gf_dd_hash_record(const uint8_t* first, int64_t L) {
  uint64_t sum = 0;
  if (L > 0) {
    const int a = (int)((uintptr_t)first & 15);
    const uint8_t* base = first - a;
    for (int64_t k = 0; 16 * k < L; ++k) {
      const gf_dd_chunk c0 = gf_dd_load_host(base, k);
      const gf_dd_chunk c1 = gf_dd_needs_next(a, L, k) ? gf_dd_load_host(base, k + 1) : gf_dd_chunk{{0, 0}};
      sum += gf_dd_piece_sum(c0, c1, a, L, k);
    }
  }
  return gf_dd_finish(L > 0 ? L : 0, sum);
}

// a key found or placed: its slot, -1 when `slots` entries were visited without success; is_new: placed by this call
inline int64_t gf_dd_place_host(uint64_t* keys, int64_t slots, uint64_t key, bool& is_new) {
  is_new = false;
  int64_t s = gf_dd_home(key, slots);
  for (int64_t t = 0; t < slots; ++t, s = gf_dd_next(s, slots)) {
    if (keys[s] == key) return s;
    if (keys[s] == 0) {
      keys[s] = key;
      is_new = true;
      return s;
    }
  }
  return -1;
}
