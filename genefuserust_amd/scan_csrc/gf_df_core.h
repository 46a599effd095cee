// The DEFLATE encoder of libgfdeflate.so, stated once: plain C++ that g++ compiles for the host (gf_df_member below:
// gf_df_member_host of include/gf_deflate.h, and tests/cpp/test_deflate_core.cpp under the sanitizers) and hipcc for
// the device (gf_df_kernels.h).  One BGZF member is encoded at a time, and its bytes are a function of its text alone:
// every choice below is arithmetic on the text, none depends on the order in which lanes run.
//
// The choices, in the order a member goes through them:
//   rounds    the text is walked in rounds of GF_DF_LANES positions.  Position p (with 4 bytes left) has the hash
//             gf_df_hash of its 4 bytes; the table holds per hash the LARGEST position + 1 inserted so far, and a round
//             reads the table before it inserts its own positions: a candidate lies in an earlier round.  Every
//             position is inserted, inside a match too.
//   match     gf_df_match_at: two candidates, the table's and distance 1 (a run), each extended up to
//             min(258, bytes left); a candidate counts from gf_df_min_len(distance) bytes on, which keeps a match from
//             costing more bits than the literals it replaces (bases code at about 2 bits, a far distance alone
//             carries 13 extra bits); the longer one wins, distance 1 on a tie.
//   tokens    greedy, no lazy evaluation: at the cursor a match is taken when there is one, else a literal.  A token
//             becomes 16-bit units: a literal one (the byte), a match two (0x4000 | length - 3, 0x8000 | distance - 1).
//             Every unit is one Huffman symbol plus its extra bits.
//   lengths   gf_df_plan: the symbols in use sorted by (count, symbol) (gf_df_rank), minimum-redundancy code lengths in
//             place (Moffat and Katajainen), limited to 15 bits (7 for the code-length code) on the counts per length,
//             the longest codes to the rarest symbols; canonical codes, stored bit-reversed for the LSB-first stream.
//   header    one final dynamic block; the code lengths are written one by one with the code-length symbols 0..15, no
//             repeat codes, all 19 code-length lengths (HCLEN 15).
//   stored    one final stored block instead, when it is not longer than the dynamic one.
//
// Bounded: every loop has a trip count fixed before it starts (rounds <= 1020, extension <= 258, the code construction
// a fixed number of passes over at most 286 symbols).
#pragma once

#include <stdint.h>

#include "gf_if_core.h"  // the CRC-32 in 64 pieces, as the inflate checks it

#define GF_DF_HD GF_IF_HD

#define GF_DF_TEXT 65280u        // text bytes per member: bgzip's
#define GF_DF_LANES 64u          // positions per round
#define GF_DF_ROUNDS 1020u       // GF_DF_TEXT / GF_DF_LANES
#define GF_DF_MAX_MATCH 258u
#define GF_DF_WINDOW 32768u
#define GF_DF_HASH_BITS 11u
#define GF_DF_HASH_SIZE (1u << GF_DF_HASH_BITS)
#define GF_DF_HEAD 18u           // the BGZF header
#define GF_DF_TAIL 8u            // CRC-32 and ISIZE
#define GF_DF_STORED_OVER 31u    // a stored member is its text and this: header, 5 bytes of block header, trailer
#define GF_DF_MEMBER_MAX (GF_DF_TEXT + GF_DF_STORED_OVER)
#define GF_DF_NLIT 286u
#define GF_DF_NDIST 30u
#define GF_DF_NSYM (GF_DF_NLIT + GF_DF_NDIST)
#define GF_DF_NCL 19u
#define GF_DF_EOB 256u
#define GF_DF_KIND_NONE 0        // no text: no member
#define GF_DF_KIND_STORED 1
#define GF_DF_KIND_DYNAMIC 2

static_assert(GF_DF_ROUNDS * GF_DF_LANES == GF_DF_TEXT && GF_DF_LANES == GF_IF_LANES, "rounds of one wavefront");
static_assert(GF_DF_MEMBER_MAX <= GF_IF_MAX_TEXT, "every member fits 64 KiB");

// ---- units and symbols ---------------------------------------------------------------------------------------------------

#define GF_DF_UNIT_LEN 0x4000u
#define GF_DF_UNIT_DIST 0x8000u

GF_DF_HD inline uint32_t gf_df_log2(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }  // x > 0

// length - 3 (0..255) -> the index of its length symbol (symbol 257 + index), its extra bits and their value
GF_DF_HD inline void gf_df_len_symbol(uint32_t l, uint32_t& index, uint32_t& extra, uint32_t& value) {
  if (l < 8u) { index = l, extra = 0, value = 0; return; }
  if (l == 255u) { index = 28, extra = 0, value = 0; return; }
  const uint32_t e = gf_df_log2(l) - 2u;
  index = 4u * e + 4u + ((l >> e) & 3u), extra = e, value = l & ((1u << e) - 1u);
}

// distance - 1 (0..32767) -> its distance symbol, its extra bits and their value
GF_DF_HD inline void gf_df_dist_symbol(uint32_t d, uint32_t& sym, uint32_t& extra, uint32_t& value) {
  if (d < 4u) { sym = d, extra = 0, value = 0; return; }
  const uint32_t e = gf_df_log2(d) - 1u;
  sym = 2u * e + 2u + ((d >> e) & 1u), extra = e, value = d & ((1u << e) - 1u);
}

GF_DF_HD inline uint32_t gf_df_len_extra(uint32_t index) { return index < 8u || index == 28u ? 0u : (index - 4u) / 4u; }
GF_DF_HD inline uint32_t gf_df_dist_extra(uint32_t sym) { return sym < 4u ? 0u : (sym - 2u) / 2u; }

// the symbol a unit counts under, in the joint numbering of GfDfPlan: literal/length 0..285, distance 286 + symbol
GF_DF_HD inline uint32_t gf_df_unit_symbol(uint32_t unit) {
  uint32_t s, e, v;
  if (unit & GF_DF_UNIT_DIST) { gf_df_dist_symbol(unit & 0x7fffu, s, e, v); return GF_DF_NLIT + s; }
  if (unit & GF_DF_UNIT_LEN) { gf_df_len_symbol(unit & 0xffu, s, e, v); return 257u + s; }
  return unit;
}

// ---- matching ------------------------------------------------------------------------------------------------------------

// the hash of the 4 bytes at p (p + 4 <= n)
GF_DF_HD inline uint32_t gf_df_hash(const uint8_t* text, uint32_t p) {
  const uint32_t v = (uint32_t)text[p] | ((uint32_t)text[p + 1] << 8) | ((uint32_t)text[p + 2] << 16) | ((uint32_t)text[p + 3] << 24);
  return (v * 2654435761u) >> (32u - GF_DF_HASH_BITS);
}

// from how many bytes on a match at `dist` is taken
GF_DF_HD inline uint32_t gf_df_min_len(uint32_t dist) {
  uint32_t s, e, v;
  gf_df_dist_symbol(dist - 1u, s, e, v);
  return 5u + (e + 1u) / 2u;
}

// 8 bytes at any address, least significant first
GF_DF_HD inline uint64_t gf_df_word(const uint8_t* p) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}

// how many bytes at c and at p agree, up to maxlen (c < p, p + maxlen <= n): eight at a time while eight are left
GF_DF_HD inline uint32_t gf_df_extend(const uint8_t* text, uint32_t c, uint32_t p, uint32_t maxlen) {
  uint32_t l = 0;
  for (uint32_t k = 0; k < (GF_DF_MAX_MATCH + 7u) / 8u; k++) {
    if (l + 8u > maxlen) break;
    const uint64_t x = gf_df_word(text + c + l) ^ gf_df_word(text + p + l);
    if (x != 0u) return l + ((uint32_t)__builtin_ctzll(x) >> 3);
    l += 8u;
  }
  for (uint32_t k = 0; k < 7u; k++) {
    if (l >= maxlen || text[c + l] != text[p + l]) break;
    l++;
  }
  return l;
}

struct GfDfMatch {
  uint32_t len, dist;  // len 0: a literal
};

// the token that starts at p < n: `entry` is what the hash table held for p's hash before p's round inserted anything
// (position + 1; 0: nothing, or fewer than 4 bytes left at p)
GF_DF_HD inline GfDfMatch gf_df_match_at(const uint8_t* text, uint32_t n, uint32_t p, uint32_t entry) {
  GfDfMatch m{0, 0};
  const uint32_t maxlen = n - p < GF_DF_MAX_MATCH ? n - p : GF_DF_MAX_MATCH;
  if (p >= 1u) {
    const uint32_t l = gf_df_extend(text, p - 1u, p, maxlen);
    if (l >= gf_df_min_len(1u)) m.len = l, m.dist = 1u;
  }
  if (entry != 0u && m.len < maxlen) {
    const uint32_t c = entry - 1u, d = p - c;  // (c lies in an earlier round: c < p)
    if (c < p && d <= GF_DF_WINDOW) {
      const uint32_t l = gf_df_extend(text, c, p, maxlen);
      if (l >= gf_df_min_len(d) && l > m.len) m.len = l, m.dist = d;
    }
  }
  return m;
}

// ---- the codes -----------------------------------------------------------------------------------------------------------

// Everything between a member's histogram and its bits.  On the device it lies in LDS and the first lane fills it.
struct GfDfPlan {
  uint32_t freq[GF_DF_NSYM];   // in: how often each symbol occurs (end-of-block included)
  uint32_t code[GF_DF_NSYM];   // (the code, bit-reversed) << 4 | its length; 0: no code
  uint32_t work[GF_DF_NLIT];
  uint16_t order[GF_DF_NSYM];  // in: the symbols in use of each alphabet by (count, symbol), ascending: gf_df_rank
  uint8_t lens[GF_DF_NSYM + 4];
  uint32_t cl_freq[GF_DF_NCL], cl_code[GF_DF_NCL];
  uint16_t cl_order[GF_DF_NCL + 1];
  uint8_t cl_lens[GF_DF_NCL + 1];
  uint32_t tally[32];          // scratch: codes per length
  uint32_t hlit, hdist;        // how many literal/length and distance code lengths the header carries
  uint32_t bits;               // of the dynamic block, header and end-of-block included
};

// the place of symbol s (freq[s] > 0) among the symbols in use of freq[0, nsym), by (count, symbol)
GF_DF_HD inline uint32_t gf_df_rank(const uint32_t* freq, uint32_t nsym, uint32_t s) {
  const uint32_t f = freq[s];
  uint32_t r = 0;
  for (uint32_t t = 0; t < nsym; t++) {
    const uint32_t g = freq[t];
    r += (g != 0u && (g < f || (g == f && t < s))) ? 1u : 0u;
  }
  return r;
}

GF_DF_HD inline void gf_df_order(const uint32_t* freq, uint32_t nsym, uint16_t* order) {
  for (uint32_t s = 0; s < nsym; s++)
    if (freq[s] != 0u) order[gf_df_rank(freq, nsym, s)] = (uint16_t)s;
}

// Code lengths of at most maxbits for the symbols of freq[0, nsym) (nsym <= GF_DF_NLIT); order: gf_df_order's; A:
// nsym words of scratch, num: 16.  No symbol in use: all 0.  One: length 1.  Else a complete code.
GF_DF_HD inline void gf_df_code_lengths(const uint32_t* freq, uint32_t nsym, const uint16_t* order, uint32_t maxbits,
                                        uint8_t* lens, uint32_t* A, uint32_t* num) {
  uint32_t n = 0;
  for (uint32_t s = 0; s < nsym; s++) {
    lens[s] = 0;
    n += freq[s] != 0u ? 1u : 0u;
  }
  if (n == 0u) return;
  if (n == 1u) { lens[order[0]] = 1; return; }
  for (uint32_t i = 0; i < n; i++) A[i] = freq[order[i]];
  // minimum redundancy in place: A[i] becomes the depth of the i-th rarest symbol
  A[0] += A[1];
  uint32_t root = 0, leaf = 2;
  for (uint32_t next = 1; next + 1u < n; next++) {
    if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; }
    else A[next] = A[leaf++];
    if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; }
    else A[next] += A[leaf++];
  }
  A[n - 2u] = 0;
  for (uint32_t k = 2; k < n; k++) {  // next = n - 3 down to 0
    const uint32_t next = n - 1u - k;
    A[next] = A[A[next]] + 1u;
  }
  {
    int32_t avbl = 1, used = 0, rt = (int32_t)n - 2, nx = (int32_t)n - 1;
    uint32_t dpth = 0;
    for (uint32_t pass = 0; pass < nsym && avbl > 0; pass++) {
      for (uint32_t k = 0; k < nsym && rt >= 0 && A[rt] == dpth; k++) { used++; rt--; }
      for (uint32_t k = 0; k < nsym && avbl > used; k++) { A[nx--] = dpth; avbl--; }
      avbl = 2 * used, dpth++, used = 0;
    }
  }
  // how many codes of each length, the lengths past maxbits counted at maxbits, then pushed down until they fit
  for (uint32_t b = 0; b < 16u; b++) num[b] = 0;
  for (uint32_t i = 0; i < n; i++) num[A[i] < maxbits ? A[i] : maxbits]++;
  uint32_t total = 0;
  for (uint32_t b = 1; b <= maxbits; b++) total += num[b] << (maxbits - b);
  for (uint32_t pass = 0; pass < 2u * GF_DF_NLIT && total > (1u << maxbits); pass++) {
    num[maxbits]--;
    for (uint32_t b = maxbits - 1u; b >= 1u; b--)
      if (num[b] != 0u) { num[b]--; num[b + 1u] += 2u; break; }
    total--;
  }
  // the rarest symbols take the longest codes
  uint32_t i = 0;
  for (uint32_t b = maxbits; b >= 1u; b--)
    for (uint32_t k = 0; k < num[b] && i < n; k++) lens[order[i++]] = (uint8_t)b;
}

// canonical codes of lens[0, nsym), bit-reversed: code[s] = reversed << 4 | length (count, next: 16 words of scratch)
GF_DF_HD inline void gf_df_codes(const uint8_t* lens, uint32_t nsym, uint32_t* code, uint32_t* count, uint32_t* next) {
  for (uint32_t b = 0; b < 16u; b++) count[b] = 0;
  for (uint32_t s = 0; s < nsym; s++) count[lens[s]]++;
  count[0] = 0;
  uint32_t c = 0;
  next[0] = 0;
  for (uint32_t b = 1; b < 16u; b++) {
    c = (c + count[b - 1u]) << 1;
    next[b] = c;
  }
  for (uint32_t s = 0; s < nsym; s++) {
    const uint32_t len = lens[s];
    if (len == 0u) { code[s] = 0; continue; }
    const uint32_t v = next[len]++;
    uint32_t r = 0;
    for (uint32_t b = 0; b < 15u; b++)
      if (b < len && ((v >> b) & 1u)) r |= 1u << (len - 1u - b);
    code[s] = (r << 4) | len;
  }
}

// the order in which a dynamic header carries the lengths of the code-length code, five bits a place (packed: a table
// indexed at run time would be a private array on the device)
constexpr uint8_t gf_df_cl_places[GF_DF_NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
constexpr uint64_t gf_df_pack5(const uint8_t (&v)[GF_DF_NCL], uint32_t from, uint32_t to) {
  uint64_t x = 0;
  for (uint32_t k = from; k < to; k++) x |= (uint64_t)v[k] << (5u * (k - from));
  return x;
}
constexpr uint64_t gf_df_cl_places_lo = gf_df_pack5(gf_df_cl_places, 0, 12), gf_df_cl_places_hi = gf_df_pack5(gf_df_cl_places, 12, GF_DF_NCL);

GF_DF_HD inline uint32_t gf_df_cl_place(uint32_t k) {
  return (uint32_t)((k < 12u ? gf_df_cl_places_lo >> (5u * k) : gf_df_cl_places_hi >> (5u * (k - 12u))) & 31u);
}

// P.freq and P.order are set: the rest of the plan
GF_DF_HD inline void gf_df_plan(GfDfPlan& P) {
  gf_df_code_lengths(P.freq, GF_DF_NLIT, P.order, 15u, P.lens, P.work, P.tally);
  gf_df_code_lengths(P.freq + GF_DF_NLIT, GF_DF_NDIST, P.order + GF_DF_NLIT, 15u, P.lens + GF_DF_NLIT, P.work, P.tally);
  uint32_t hlit = 257u, hdist = 1u;
  for (uint32_t s = 257u; s < GF_DF_NLIT; s++)
    if (P.lens[s] != 0u) hlit = s + 1u;
  for (uint32_t s = 1u; s < GF_DF_NDIST; s++)
    if (P.lens[GF_DF_NLIT + s] != 0u) hdist = s + 1u;
  P.hlit = hlit, P.hdist = hdist;
  for (uint32_t k = 0; k < GF_DF_NCL; k++) P.cl_freq[k] = 0;
  for (uint32_t s = 0; s < hlit; s++) P.cl_freq[P.lens[s]]++;
  for (uint32_t s = 0; s < hdist; s++) P.cl_freq[P.lens[GF_DF_NLIT + s]]++;
  // (a code of one symbol would be incomplete, which no decoder takes for this code: a second one joins it)
  uint32_t in_use = 0;
  for (uint32_t k = 0; k < 16u; k++) in_use += P.cl_freq[k] != 0u ? 1u : 0u;
  if (in_use == 1u) P.cl_freq[P.cl_freq[0] != 0u ? 1 : 0] = 1;
  gf_df_order(P.cl_freq, GF_DF_NCL, P.cl_order);
  gf_df_code_lengths(P.cl_freq, GF_DF_NCL, P.cl_order, 7u, P.cl_lens, P.work, P.tally);
  gf_df_codes(P.lens, GF_DF_NLIT, P.code, P.tally, P.tally + 16);
  gf_df_codes(P.lens + GF_DF_NLIT, GF_DF_NDIST, P.code + GF_DF_NLIT, P.tally, P.tally + 16);
  gf_df_codes(P.cl_lens, GF_DF_NCL, P.cl_code, P.tally, P.tally + 16);
  uint32_t bits = 3u + 5u + 5u + 4u + 3u * GF_DF_NCL;
  for (uint32_t s = 0; s < hlit; s++) bits += P.cl_lens[P.lens[s]];
  for (uint32_t s = 0; s < hdist; s++) bits += P.cl_lens[P.lens[GF_DF_NLIT + s]];
  for (uint32_t s = 0; s < GF_DF_NLIT; s++)
    bits += P.freq[s] * (P.lens[s] + (s > 256u ? gf_df_len_extra(s - 257u) : 0u));
  for (uint32_t s = 0; s < GF_DF_NDIST; s++) bits += P.freq[GF_DF_NLIT + s] * (P.lens[GF_DF_NLIT + s] + gf_df_dist_extra(s));
  P.bits = bits;
}

// the kind of the member of n > 0 text bytes whose dynamic block takes `bits`, and its payload bytes
GF_DF_HD inline int gf_df_kind(uint32_t n, uint32_t bits, uint32_t& payload) {
  const uint32_t dynamic = (bits + 7u) / 8u, stored = n + 5u;
  payload = stored <= dynamic ? stored : dynamic;
  return stored <= dynamic ? GF_DF_KIND_STORED : GF_DF_KIND_DYNAMIC;
}

// The dynamic block's header through put(bit position, value, bits), from bit position `at` on; returns where the
// first unit's bits go.  A value goes in with its least significant bit first.
template <typename Put>
GF_DF_HD inline uint32_t gf_df_block_header(const GfDfPlan& P, uint32_t at, Put& put) {
  put(at, 1u | (2u << 1), 3u), at += 3u;  // final, dynamic
  put(at, P.hlit - 257u, 5u), at += 5u;
  put(at, P.hdist - 1u, 5u), at += 5u;
  put(at, GF_DF_NCL - 4u, 4u), at += 4u;
  for (uint32_t k = 0; k < GF_DF_NCL; k++) put(at, P.cl_lens[gf_df_cl_place(k)], 3u), at += 3u;
  for (uint32_t s = 0; s < P.hlit + P.hdist; s++) {
    const uint32_t c = P.cl_code[P.lens[s < P.hlit ? s : GF_DF_NLIT + s - P.hlit]];
    put(at, c >> 4, c & 15u), at += c & 15u;
  }
  return at;
}

// a unit's bits (the symbol's code, then its extra bits) and how many
GF_DF_HD inline uint32_t gf_df_unit_bits(const uint32_t* code, uint32_t unit, uint32_t& nbits) {
  uint32_t s, e = 0, v = 0, c;
  if (unit & GF_DF_UNIT_DIST) { gf_df_dist_symbol(unit & 0x7fffu, s, e, v); c = code[GF_DF_NLIT + s]; }
  else if (unit & GF_DF_UNIT_LEN) { gf_df_len_symbol(unit & 0xffu, s, e, v); c = code[257u + s]; }
  else c = code[unit];
  nbits = (c & 15u) + e;
  return (c >> 4) | (v << (c & 15u));
}

// ---- the frame -----------------------------------------------------------------------------------------------------------

// byte k < 18 of the header of a member of `size` bytes in all
GF_DF_HD inline uint8_t gf_df_head_byte(uint32_t k, uint32_t size) {
  // 1f 8b 08 04 00000000 | 00 ff 0600 'B' 'C' 0200, least significant byte first
  if (k < 8u) return (uint8_t)(0x0000000004088b1full >> (8u * k));
  if (k < 16u) return (uint8_t)(0x000243420006ff00ull >> (8u * (k - 8u)));
  return (uint8_t)((size - 1u) >> (8u * (k - 16u)));
}

// byte k < 8 of the trailer
GF_DF_HD inline uint8_t gf_df_tail_byte(uint32_t k, uint32_t crc, uint32_t n) {
  return (uint8_t)((k < 4u ? crc : n) >> (8u * (k & 3u)));
}

// byte k of the stored member of text[0, n)
GF_DF_HD inline uint8_t gf_df_stored_byte(uint32_t k, const uint8_t* text, uint32_t n, uint32_t crc) {
  const uint32_t size = n + GF_DF_STORED_OVER;
  if (k < GF_DF_HEAD) return gf_df_head_byte(k, size);
  if (k >= size - GF_DF_TAIL) return gf_df_tail_byte(k - (size - GF_DF_TAIL), crc, n);
  const uint32_t q = k - GF_DF_HEAD;
  if (q == 0u) return 1;  // final, stored, and the bits up to the byte's end
  if (q < 5u) return (uint8_t)((q < 3u ? n : ~n) >> (8u * ((q - 1u) & 1u)));
  return text[q - 5u];
}

// the CRC-32 of text[0, n), the way the device takes it: in pieces, joined (table: gf_if_crc_table_entry's 256)
GF_DF_HD inline uint32_t gf_df_crc_serial(const uint32_t* table, const uint8_t* text, uint32_t n) {
  uint32_t pieces[GF_IF_LANES];
  for (uint32_t k = 0; k < GF_IF_LANES; k++) pieces[k] = gf_if_crc_piece(table, text, n, k);
  return gf_if_crc_join(pieces, n);
}

// ---- the member on the host: the device's rounds, one lane after the other ------------------------------------------------

struct GfDfHostBits {
  uint8_t* out;  // zeroed
  void operator()(uint32_t at, uint32_t value, uint32_t bits) {
    for (uint32_t b = 0; b < bits; b++)
      if ((value >> b) & 1u) out[(at + b) >> 3] |= (uint8_t)(1u << ((at + b) & 7u));
  }
};

// The member of text[0, n), 0 < n <= GF_DF_TEXT, into out[0, GF_DF_MEMBER_MAX): returns its size; kind: GF_DF_KIND_*.
// units: GF_DF_TEXT 16-bit units of scratch, table: GF_DF_HASH_SIZE words of scratch.
inline uint32_t gf_df_member(const uint8_t* text, uint32_t n, uint8_t* out, uint16_t* units, uint32_t* table, int& kind) {
  uint32_t crc_table[256];
  for (uint32_t i = 0; i < 256u; i++) crc_table[i] = gf_if_crc_table_entry(i);
  const uint32_t crc = gf_df_crc_serial(crc_table, text, n);
  GfDfPlan P;
  for (uint32_t s = 0; s < GF_DF_NSYM; s++) P.freq[s] = 0;
  for (uint32_t h = 0; h < GF_DF_HASH_SIZE; h++) table[h] = 0;
  uint32_t cur = 0, n_units = 0;
  const uint32_t rounds = (n + GF_DF_LANES - 1u) / GF_DF_LANES;
  for (uint32_t r = 0; r < rounds; r++) {
    const uint32_t base = r * GF_DF_LANES;
    uint32_t entry[GF_DF_LANES];
    for (uint32_t lane = 0; lane < GF_DF_LANES; lane++) {
      const uint32_t p = base + lane;
      entry[lane] = p + 4u <= n ? table[gf_df_hash(text, p)] : 0u;
    }
    for (uint32_t lane = 0; lane < GF_DF_LANES; lane++) {
      const uint32_t p = base + lane;
      if (p + 4u <= n) {
        uint32_t& e = table[gf_df_hash(text, p)];
        if (e < p + 1u) e = p + 1u;
      }
    }
    const uint32_t end = base + GF_DF_LANES < n ? base + GF_DF_LANES : n;
    for (uint32_t k = 0; k < GF_DF_LANES && cur < end; k++) {
      const GfDfMatch m = gf_df_match_at(text, n, cur, entry[cur - base]);
      if (m.len != 0u) {
        units[n_units++] = (uint16_t)(GF_DF_UNIT_LEN | (m.len - 3u));
        units[n_units++] = (uint16_t)(GF_DF_UNIT_DIST | (m.dist - 1u));
        cur += m.len;
      } else {
        units[n_units++] = text[cur];
        cur++;
      }
    }
  }
  for (uint32_t u = 0; u < n_units; u++) P.freq[gf_df_unit_symbol(units[u])]++;
  P.freq[GF_DF_EOB]++;
  gf_df_order(P.freq, GF_DF_NLIT, P.order);
  gf_df_order(P.freq + GF_DF_NLIT, GF_DF_NDIST, P.order + GF_DF_NLIT);
  gf_df_plan(P);
  uint32_t payload;
  kind = gf_df_kind(n, P.bits, payload);
  const uint32_t size = GF_DF_HEAD + payload + GF_DF_TAIL;
  if (kind == GF_DF_KIND_STORED) {
    for (uint32_t k = 0; k < size; k++) out[k] = gf_df_stored_byte(k, text, n, crc);
    return size;
  }
  for (uint32_t k = 0; k < size; k++) out[k] = 0;
  GfDfHostBits put{out};
  uint32_t at = gf_df_block_header(P, 8u * GF_DF_HEAD, put);
  for (uint32_t u = 0; u < n_units; u++) {
    uint32_t nbits;
    const uint32_t v = gf_df_unit_bits(P.code, units[u], nbits);
    put(at, v, nbits), at += nbits;
  }
  put(at, P.code[GF_DF_EOB] >> 4, P.code[GF_DF_EOB] & 15u);
  for (uint32_t k = 0; k < GF_DF_HEAD; k++) out[k] = gf_df_head_byte(k, size);
  for (uint32_t k = 0; k < GF_DF_TAIL; k++) out[size - GF_DF_TAIL + k] = gf_df_tail_byte(k, crc, n);
  return size;
}
