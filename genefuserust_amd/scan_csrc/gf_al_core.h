// The whole-genome alignable filter of libgfalign.so, the arithmetic written once: plain C++ that g++ compiles for the
// host (tests/cpp/test_alignable_core.cpp, under the sanitizers) and hipcc for the device (gf_al_kernels.h).
//
//   the predicate     a strand string s of length L lies on the diagonal p of a reference text c: position i matches
//                     when s[i] == upper(c[p + i]) and that byte is one of ACGT; it is covered when it lies in a window
//                     of GF_AL_K positions that all match, that is, in a run of at least GF_AL_K matches; the diagonal
//                     is alignable when fewer than GF_AL_LIMIT positions are uncovered
//   the strands       s = 2 r + t is strand t of read r: t = 0 the read as it is, t = 1 its reverse complement as
//                     fusion_mapper.reverse_complement makes it (anything outside ACGTacgt becomes N, upper case)
//   the seeds         the 2-bit key of a window, a seed's 63 bits {key, string, offset}, the filter's hash, a key's bucket
//
// Every loop is bounded by a length its caller checked; nothing outside [0, len) of the string or [0, text_bytes) of the
// text is read.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define GF_AL_HD __host__ __device__
#else
#define GF_AL_HD
#endif

#define GF_AL_K 16                      // matcher.rs:30
#define GF_AL_LIMIT 10                  // matcher.rs:516: mismatches.len() < 10
#define GF_AL_MAX_LEN 4096              // GF_MAX_READ_LEN: a seed's offset has 12 bits
#define GF_AL_MAX_READS (1 << 18)       // a seed's string has 19 bits: two strands a read
#define GF_AL_BUCKET_BITS 18            // the sorted seeds are entered through the first 9 bases of their key
#define GF_AL_MIN_FILTER_LOG2 16        // the membership filter has 2^16 .. 2^32 bits (2^32: exact, no hash)
#define GF_AL_MAX_FILTER_LOG2 32
#define GF_AL_SEPARATOR 0               // the byte between two contigs of a piece: no alignment holds one
#define GF_AL_NO_SEED INT64_MAX         // a slot without a seed: sorts behind every seed

// 0 .. 3 for ACGT, 4 for every other byte (lower case too: a read is compared as it is)
GF_AL_HD inline uint32_t gf_al_code(uint8_t b) {
  return b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : 4u;
}

// u8::to_ascii_uppercase (matcher.rs:141)
GF_AL_HD inline uint8_t gf_al_upper(uint8_t b) { return b >= 'a' && b <= 'z' ? (uint8_t)(b - 32) : b; }

// position i of the predicate: the string's byte against the text's
GF_AL_HD inline bool gf_al_match(uint8_t s, uint8_t c) { return s == gf_al_upper(c) && gf_al_code(s) < 4u; }

// a byte of the reverse complement (sequence.rs:22-60)
GF_AL_HD inline uint8_t gf_al_complement(uint8_t b) {
  switch (b) {
    case 'A': case 'a': return 'T';
    case 'C': case 'c': return 'G';
    case 'G': case 'g': return 'C';
    case 'T': case 't': return 'A';
    default: return 'N';
  }
}

// Strand string s of the reads back to back in `bases`: read r = s >> 1 is bases[start, start + len); the strings lie
// back to back too, both strands of a read next to each other, so string s starts at 2 * start + (s & 1) * len.
GF_AL_HD inline int64_t gf_al_string_start(int64_t read_start, int64_t len, int64_t s) { return 2 * read_start + (s & 1) * len; }

// ---- seeds -------------------------------------------------------------------------------------------------------------

// {key: 32, string: 19, offset: 12}: never negative, so the order of int64 is the order of the keys
GF_AL_HD inline int64_t gf_al_seed(uint32_t key, uint32_t string, uint32_t offset) {
  return (int64_t)(((uint64_t)key << 31) | ((uint64_t)string << 12) | offset);
}
GF_AL_HD inline uint32_t gf_al_seed_key(int64_t seed) { return (uint32_t)((uint64_t)seed >> 31); }
GF_AL_HD inline uint32_t gf_al_seed_string(int64_t seed) { return (uint32_t)((uint64_t)seed >> 12) & 0x7FFFFu; }
GF_AL_HD inline uint32_t gf_al_seed_offset(int64_t seed) { return (uint32_t)seed & 0xFFFu; }

GF_AL_HD inline uint32_t gf_al_bucket(uint32_t key) { return key >> (32 - GF_AL_BUCKET_BITS); }

// the filter's bit of a key: the key itself in a map of 2^32 bits, else the top bits of a multiplicative hash
GF_AL_HD inline uint32_t gf_al_filter_bit(uint32_t key, int32_t log2_bits) {
  return log2_bits >= 32 ? key : (uint32_t)(key * 0x9E3779B1u) >> (32 - log2_bits);
}

// The key of the window s[j, j + GF_AL_K) of a string; false when a byte of it is outside ACGT.
GF_AL_HD inline bool gf_al_window_key(const uint8_t* s, int64_t j, uint32_t& key) {
  uint32_t k = 0;
  for (int32_t i = 0; i < GF_AL_K; i++) {
    const uint32_t c = gf_al_code(s[j + i]);
    if (c > 3u) return false;
    k = (k << 2) | c;
  }
  key = k;
  return true;
}

// ---- the predicate on one diagonal -------------------------------------------------------------------------------------

// Whether string s[0, len) is alignable on the diagonal p of text[0, text_bytes): fewer than GF_AL_LIMIT positions
// outside every run of at least GF_AL_K matches.  False when the string is shorter than GF_AL_K, when [p, p + len)
// does not lie inside the text, and when it holds a GF_AL_SEPARATOR (an alignment never spans two contigs).  Stops at
// the GF_AL_LIMIT-th uncovered position.
GF_AL_HD inline bool gf_al_diagonal(const uint8_t* s, int64_t len, const uint8_t* text, int64_t text_bytes, int64_t p) {
  if (len < GF_AL_K || len > GF_AL_MAX_LEN || p < 0 || p > text_bytes - len) return false;
  const uint8_t* c = text + p;
  int32_t uncovered = 0;   // positions outside a run, or in a closed run shorter than GF_AL_K
  int32_t run = 0;         // the matches that end at i - 1
  for (int64_t i = 0; i < len; i++) {
    const uint8_t t = c[i];
    if (gf_al_match(s[i], t)) {
      run++;
      continue;
    }
    if (t == GF_AL_SEPARATOR) return false;
    uncovered += 1 + (run < GF_AL_K ? run : 0);
    run = 0;
    if (uncovered >= GF_AL_LIMIT) return false;
  }
  if (run < GF_AL_K) uncovered += run;
  return uncovered < GF_AL_LIMIT;
}

// The number of uncovered positions of the same diagonal, without the early stop (the host tests compare it with the
// model's); -1 where gf_al_diagonal refuses the diagonal.
GF_AL_HD inline int32_t gf_al_uncovered(const uint8_t* s, int64_t len, const uint8_t* text, int64_t text_bytes, int64_t p) {
  if (len < GF_AL_K || len > GF_AL_MAX_LEN || p < 0 || p > text_bytes - len) return -1;
  int32_t uncovered = 0, run = 0;
  for (int64_t i = 0; i < len; i++) {
    const uint8_t t = text[p + i];
    if (gf_al_match(s[i], t)) {
      run++;
      continue;
    }
    if (t == GF_AL_SEPARATOR) return -1;
    uncovered += 1 + (run < GF_AL_K ? run : 0);
    run = 0;
  }
  if (run < GF_AL_K) uncovered += run;
  return uncovered;
}

// Whether the seed at offset j of string s opens an exact run on the diagonal through text position g (the window's
// first base): j == 0, or the base before the window does not match.  A diagonal is tested from such seeds only.
GF_AL_HD inline bool gf_al_opens_run(const uint8_t* s, int64_t j, const uint8_t* text, int64_t g) {
  return j == 0 || g == 0 || !gf_al_match(s[j - 1], text[g - 1]);
}
