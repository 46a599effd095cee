// The DEFLATE decoder of libgfinflate.so, written once: plain C++ that g++ compiles for the host (tests/cpp/
// test_inflate_core.cpp, under the sanitizers) and hipcc for the device (gf_if_kernels.h).  One BGZF member is decoded
// at a time: its payload is raw DEFLATE, it shares no window with its neighbours, and its text length (ISIZE) and
// CRC-32 are known from its trailer before the first bit is read.
//
// On the device the whole wavefront runs this text with the same values: every value read from memory goes through
// GF_IF_UNIFORM (the first lane's copy, so that the compiler keeps the decoder's state in scalar registers), every store
// to the tables is the first lane's alone (GF_IF_STORE).  Where the bytes go is the Sink's business — the only part
// that differs between host and device:
//     sink.put(pos, byte)          a literal
//     sink.raw(pos, src, len)      len bytes of a stored block
//     sink.copy(pos, dist, len)    a match: byte pos + i is byte pos - dist + (i % dist)
//
// Bounded by construction: every iteration of every loop consumes at least one payload bit or produces at least one
// byte of text, or has a fixed trip count; a bit past the payload's end or a byte past ISIZE ends the decode with a
// status.  Nothing a Sink is asked to write lies outside [0, isize), nothing it is asked to read outside [0, pos) or the
// payload.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define GF_IF_HD __host__ __device__
#define GF_IF_UNROLL _Pragma("unroll")
#else
#define GF_IF_HD
#define GF_IF_UNROLL
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define GF_IF_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#define GF_IF_LEADER (threadIdx.x == 0)
#else
#define GF_IF_UNIFORM(x) ((uint32_t)(x))
#define GF_IF_LEADER true
#endif
#define GF_IF_STORE(lvalue, v)          \
  do {                                  \
    if (GF_IF_LEADER) (lvalue) = (v);   \
  } while (0)

// the status of a member (int32 per member in gf_if_inflate_device's d_status; include/gf_inflate.h names them too)
#define GF_IF_OK 0
#define GF_IF_BAD_BTYPE 1          // reserved block type 3
#define GF_IF_STORED_LEN 2         // stored block: LEN != ~NLEN
#define GF_IF_BAD_COUNTS 3         // HLIT > 286 or HDIST > 30
#define GF_IF_OVERSUBSCRIBED 4     // a code with more codes than its lengths allow
#define GF_IF_INCOMPLETE 5         // an incomplete code (other than a distance code of one length-1 code, or of none)
#define GF_IF_REPEAT_FIRST 6       // repeat code 16 with no length before it
#define GF_IF_LENGTHS_OVERRUN 7    // a repeat runs past HLIT + HDIST
#define GF_IF_NO_END_CODE 8        // the end-of-block symbol has no code
#define GF_IF_BAD_LITLEN 9         // literal/length symbol 286 or 287
#define GF_IF_BAD_DIST_SYM 10      // distance symbol 30 or 31
#define GF_IF_DIST_TOO_FAR 11      // a distance beyond what this member has produced
#define GF_IF_OUTPUT_OVERRUN 12    // more text than ISIZE
#define GF_IF_OUTPUT_SHORT 13      // less text than ISIZE
#define GF_IF_INPUT_EXHAUSTED 14   // the payload ends inside the stream
#define GF_IF_CRC 15               // the text's CRC-32 is not the trailer's
#define GF_IF_BAD_ROW 16           // the table row points outside the compressed bytes or the output, or past 64 KiB
#define GF_IF_BAD_CODE 17          // bits that are no code of an incomplete code
#define GF_IF_TRAILING 18          // payload bytes left behind the final block

#define GF_IF_MAX_TEXT 65536       // a BGZF member holds at most 64 KiB of text, and is itself at most 64 KiB long
#define GF_IF_ROW 6                // int64 per table row: payload offset, payload length, text offset, text length
                                   // (ISIZE), CRC-32, the member's offset in the file
#define GF_IF_LANES 64             // the CRC is taken in this many pieces and joined

struct GfIfTables {
  uint16_t lit_count[16], lit_sym[288];
  uint16_t dist_count[16], dist_sym[32];
  uint16_t len_count[16], len_sym[20];
  uint16_t offs[16];
  uint8_t lengths[320];
};

// ---- the LSB-first bit reader ------------------------------------------------------------------------------------------

struct GfIfBits {
  const uint8_t* p;
  uint32_t n_bytes, n_bits;  // of the payload
  uint32_t used;             // bits consumed
  uint32_t next;             // the next byte to load
  uint32_t cnt;              // bits in buf (zeros stand in past the payload's end; `used` is what is checked)
  uint64_t buf;
};

GF_IF_HD inline void gf_if_bits_init(GfIfBits& b, const uint8_t* p, uint32_t n_bytes) {
  b.p = p, b.n_bytes = n_bytes, b.n_bits = 8 * n_bytes;
  b.used = 0, b.next = 0, b.cnt = 0, b.buf = 0;
}

// at least 57 bits in buf: at most 8 loads
GF_IF_HD inline void gf_if_fill(GfIfBits& b) {
  while (b.cnt <= 56) {
    const uint32_t v = b.next < b.n_bytes ? GF_IF_UNIFORM(b.p[b.next]) : 0u;
    b.buf |= (uint64_t)v << b.cnt;
    b.next++;
    b.cnt += 8;
  }
}

// consumes k <= 32 bits that gf_if_fill has put into buf; false when the payload does not have them
GF_IF_HD inline bool gf_if_take(GfIfBits& b, uint32_t k) {
  if (b.used + k > b.n_bits) return false;
  b.used += k;
  b.buf >>= k;
  b.cnt -= k;
  return true;
}

// the next k <= 16 bits as a number
GF_IF_HD inline bool gf_if_bits(GfIfBits& b, uint32_t k, uint32_t& v) {
  if (b.cnt < k) gf_if_fill(b);
  v = (uint32_t)b.buf & ((1u << k) - 1u);
  return gf_if_take(b, k);
}

// ---- canonical codes ---------------------------------------------------------------------------------------------------

// count[len] codes of each length and the symbols in code order, from n code lengths.  Returns what is left of the code
// space: 0 complete, > 0 incomplete, < 0 over-subscribed (nothing of `symbol` is written then).
GF_IF_HD inline int gf_if_construct(uint16_t* count, uint16_t* symbol, uint16_t* offs, const uint8_t* lengths, uint32_t n) {
  for (uint32_t len = 0; len < 16; len++) GF_IF_STORE(count[len], (uint16_t)0);
  for (uint32_t s = 0; s < n; s++) {
    const uint32_t l = GF_IF_UNIFORM(lengths[s]) & 15u;
    const uint32_t c = GF_IF_UNIFORM(count[l]);
    GF_IF_STORE(count[l], (uint16_t)(c + 1));
  }
  int left = 1;
  for (uint32_t len = 1; len < 16; len++) {
    left <<= 1;
    left -= (int)GF_IF_UNIFORM(count[len]);
    if (left < 0) return left;
  }
  GF_IF_STORE(offs[1], (uint16_t)0);
  for (uint32_t len = 1; len < 15; len++) {
    const uint32_t o = GF_IF_UNIFORM(offs[len]) + GF_IF_UNIFORM(count[len]);
    GF_IF_STORE(offs[len + 1], (uint16_t)o);
  }
  for (uint32_t s = 0; s < n; s++) {
    const uint32_t l = GF_IF_UNIFORM(lengths[s]) & 15u;
    if (l == 0) continue;
    const uint32_t o = GF_IF_UNIFORM(offs[l]);  // (below n: the code is not over-subscribed)
    GF_IF_STORE(symbol[o], (uint16_t)s);
    GF_IF_STORE(offs[l], (uint16_t)(o + 1));
  }
  return left;
}

// A code's counts per length by value: uniform, and indexed by unrolled loops only, so that the device keeps them in
// scalar registers and a symbol costs one look-up in LDS, not one per bit.
struct GfIfCounts {
  uint32_t c[16];
};

GF_IF_HD inline GfIfCounts gf_if_counts(const uint16_t* count) {
  GfIfCounts k;
  GF_IF_UNROLL
  for (uint32_t len = 0; len < 16; len++) k.c[len] = GF_IF_UNIFORM(count[len]);
  return k;
}

// The next symbol: one bit per iteration, at most 15.  A negative status when the bits are no code or the payload ends.
GF_IF_HD inline int gf_if_decode(GfIfBits& b, const GfIfCounts& count, const uint16_t* symbol) {
  if (b.cnt < 15) gf_if_fill(b);
  uint32_t w = (uint32_t)b.buf;
  int code = 0, first = 0, index = 0;
  GF_IF_UNROLL
  for (uint32_t len = 1; len <= 15; len++) {
    code |= (int)(w & 1u);
    w >>= 1;
    const int c = (int)count.c[len];
    if (code - c < first) {
      if (!gf_if_take(b, len)) return -GF_IF_INPUT_EXHAUSTED;
      return (int)GF_IF_UNIFORM(symbol[index + (code - first)]);
    }
    index += c;
    first += c;
    first <<= 1;
    code <<= 1;
  }
  return -GF_IF_BAD_CODE;
}

// ---- the three kinds of block -------------------------------------------------------------------------------------------

template <class Sink>
GF_IF_HD inline int gf_if_stored(GfIfBits& b, uint32_t& pos, uint32_t isize, Sink& sink) {
  if (!gf_if_take(b, (8u - (b.used & 7u)) & 7u)) return GF_IF_INPUT_EXHAUSTED;  // (cnt is a multiple of 8 less `used`'s odd bits)
  uint32_t len = 0, nlen = 0;
  if (!gf_if_bits(b, 16, len) || !gf_if_bits(b, 16, nlen)) return GF_IF_INPUT_EXHAUSTED;
  if (len != (~nlen & 0xffffu)) return GF_IF_STORED_LEN;
  if (b.used + 8 * len > b.n_bits) return GF_IF_INPUT_EXHAUSTED;
  if (pos + len > isize) return GF_IF_OUTPUT_OVERRUN;
  sink.raw(pos, b.p + (b.used >> 3), len);
  pos += len;
  b.used += 8 * len;
  b.next = b.used >> 3, b.cnt = 0, b.buf = 0;
  return GF_IF_OK;
}

GF_IF_HD inline int gf_if_fixed_tables(GfIfTables& T) {
  for (uint32_t s = 0; s < 288; s++) GF_IF_STORE(T.lengths[s], (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8));
  gf_if_construct(T.lit_count, T.lit_sym, T.offs, T.lengths, 288);
  for (uint32_t s = 0; s < 32; s++) GF_IF_STORE(T.lengths[s], (uint8_t)5);
  gf_if_construct(T.dist_count, T.dist_sym, T.offs, T.lengths, 32);
  return GF_IF_OK;
}

GF_IF_HD inline int gf_if_dynamic_tables(GfIfBits& b, GfIfTables& T) {
  static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint32_t nlen = 0, ndist = 0, ncode = 0;
  if (!gf_if_bits(b, 5, nlen) || !gf_if_bits(b, 5, ndist) || !gf_if_bits(b, 4, ncode)) return GF_IF_INPUT_EXHAUSTED;
  nlen += 257, ndist += 1, ncode += 4;
  if (nlen > 286 || ndist > 30) return GF_IF_BAD_COUNTS;
  for (uint32_t i = 0; i < 19; i++) {
    uint32_t v = 0;
    if (i < ncode && !gf_if_bits(b, 3, v)) return GF_IF_INPUT_EXHAUSTED;
    GF_IF_STORE(T.lengths[order[i]], (uint8_t)v);
  }
  int left = gf_if_construct(T.len_count, T.len_sym, T.offs, T.lengths, 19);
  if (left != 0) return left < 0 ? GF_IF_OVERSUBSCRIBED : GF_IF_INCOMPLETE;
  const uint32_t total = nlen + ndist;
  const GfIfCounts len_count = gf_if_counts(T.len_count);
  uint32_t idx = 0;
  while (idx < total) {  // (every iteration consumes a code)
    const int sym = gf_if_decode(b, len_count, T.len_sym);
    if (sym < 0) return -sym;
    if (sym < 16) {
      GF_IF_STORE(T.lengths[idx], (uint8_t)sym);
      idx++;
      continue;
    }
    uint32_t prev = 0, rep = 0;
    if (sym == 16) {
      if (idx == 0) return GF_IF_REPEAT_FIRST;
      prev = GF_IF_UNIFORM(T.lengths[idx - 1]);
      if (!gf_if_bits(b, 2, rep)) return GF_IF_INPUT_EXHAUSTED;
      rep += 3;
    } else if (sym == 17) {
      if (!gf_if_bits(b, 3, rep)) return GF_IF_INPUT_EXHAUSTED;
      rep += 3;
    } else {
      if (!gf_if_bits(b, 7, rep)) return GF_IF_INPUT_EXHAUSTED;
      rep += 11;
    }
    if (idx + rep > total) return GF_IF_LENGTHS_OVERRUN;
    for (uint32_t k = 0; k < rep; k++) GF_IF_STORE(T.lengths[idx + k], (uint8_t)prev);
    idx += rep;
  }
  if (GF_IF_UNIFORM(T.lengths[256]) == 0) return GF_IF_NO_END_CODE;
  left = gf_if_construct(T.lit_count, T.lit_sym, T.offs, T.lengths, nlen);
  if (left != 0) return left < 0 ? GF_IF_OVERSUBSCRIBED : GF_IF_INCOMPLETE;
  left = gf_if_construct(T.dist_count, T.dist_sym, T.offs, T.lengths + nlen, ndist);
  if (left < 0) return GF_IF_OVERSUBSCRIBED;
  // incomplete is allowed where every distance code is at most one bit long: one code of length 1, or none at all
  if (left > 0 && GF_IF_UNIFORM(T.dist_count[0]) + GF_IF_UNIFORM(T.dist_count[1]) != ndist) return GF_IF_INCOMPLETE;
  return GF_IF_OK;
}

// the symbols of a fixed or dynamic block up to its end-of-block code
template <class Sink>
GF_IF_HD inline int gf_if_codes(GfIfBits& b, const GfIfTables& T, uint32_t& pos, uint32_t isize, Sink& sink) {
  static const uint16_t len_base[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                        31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
  static const uint8_t len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
  static const uint16_t dist_base[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
                                         193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
  static const uint8_t dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
  const GfIfCounts lit_count = gf_if_counts(T.lit_count), dist_count = gf_if_counts(T.dist_count);
  for (;;) {  // (every iteration consumes a code)
    int sym = gf_if_decode(b, lit_count, T.lit_sym);
    if (sym < 0) return -sym;
    if (sym < 256) {
      if (pos >= isize) return GF_IF_OUTPUT_OVERRUN;
      sink.put(pos, (uint8_t)sym);
      pos++;
      continue;
    }
    if (sym == 256) return GF_IF_OK;
    sym -= 257;
    if (sym >= 29) return GF_IF_BAD_LITLEN;
    uint32_t extra = 0;
    if (!gf_if_bits(b, len_extra[sym], extra)) return GF_IF_INPUT_EXHAUSTED;
    const uint32_t len = len_base[sym] + extra;
    const int dsym = gf_if_decode(b, dist_count, T.dist_sym);
    if (dsym < 0) return -dsym;
    if (dsym >= 30) return GF_IF_BAD_DIST_SYM;
    if (!gf_if_bits(b, dist_extra[dsym], extra)) return GF_IF_INPUT_EXHAUSTED;
    const uint32_t dist = dist_base[dsym] + extra;
    if (dist > pos) return GF_IF_DIST_TOO_FAR;
    if (pos + len > isize) return GF_IF_OUTPUT_OVERRUN;
    sink.copy(pos, dist, len);
    pos += len;
  }
}

// One member's payload into its text, CRC aside: GF_IF_OK when exactly isize bytes came out of exactly the payload.
template <class Sink>
GF_IF_HD inline int gf_if_inflate_member(const uint8_t* payload, uint32_t n_bytes, uint32_t isize, GfIfTables& T, Sink& sink) {
  GfIfBits b;
  gf_if_bits_init(b, payload, n_bytes);
  uint32_t pos = 0, last = 0;
  while (!last) {  // (every iteration consumes a block header)
    uint32_t type = 0;
    if (!gf_if_bits(b, 1, last) || !gf_if_bits(b, 2, type)) return GF_IF_INPUT_EXHAUSTED;
    int st;
    if (type == 0) {
      st = gf_if_stored(b, pos, isize, sink);
    } else if (type == 3) {
      st = GF_IF_BAD_BTYPE;
    } else {
      st = type == 1 ? gf_if_fixed_tables(T) : gf_if_dynamic_tables(b, T);
      if (st == GF_IF_OK) st = gf_if_codes(b, T, pos, isize, sink);
    }
    if (st != GF_IF_OK) return st;
  }
  if (pos != isize) return GF_IF_OUTPUT_SHORT;
  if (((b.used + 7) >> 3) != n_bytes) return GF_IF_TRAILING;
  return GF_IF_OK;
}

// Whether a table row may be decoded at all: inside the compressed bytes, inside the output, and no larger than a BGZF
// member can be.
GF_IF_HD inline bool gf_if_row_ok(const int64_t* row, int64_t comp_bytes, int64_t out_cap) {
  const int64_t po = row[0], pl = row[1], to = row[2], tl = row[3];
  if (po < 0 || pl < 0 || pl > GF_IF_MAX_TEXT || po > comp_bytes - pl) return false;
  if (to < 0 || tl < 0 || tl > GF_IF_MAX_TEXT || to > out_cap - tl) return false;
  return true;
}

// ---- CRC-32 ------------------------------------------------------------------------------------------------------------
// The text's CRC is taken in GF_IF_LANES pieces — on the device a lane each — and joined: piece k is the text's
// [n - (LANES - k) * seg, n - (LANES - 1 - k) * seg), cut at 0, with seg = ceil(n / LANES), so that only the first
// pieces are short or empty and one factor x^(8 seg) joins them all.

GF_IF_HD inline uint32_t gf_if_crc_table_entry(uint32_t i) {
  uint32_t c = i;
  for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
  return c;
}

GF_IF_HD inline uint32_t gf_if_crc_seg(uint32_t n) { return (n + GF_IF_LANES - 1) / GF_IF_LANES; }

// the CRC-32 of piece `lane` of text[0, n)
GF_IF_HD inline uint32_t gf_if_crc_piece(const uint32_t* table, const uint8_t* text, uint32_t n, uint32_t lane) {
  const uint32_t seg = gf_if_crc_seg(n);
  const int64_t lo = (int64_t)n - (int64_t)(GF_IF_LANES - lane) * seg, hi = lo + seg;
  uint32_t c = 0xffffffffu;
  for (int64_t i = lo < 0 ? 0 : lo; i < hi; i++) c = table[(c ^ text[i]) & 0xffu] ^ (c >> 8);
  return c ^ 0xffffffffu;
}

// a * b mod P, polynomials over GF(2) in the CRC's reflected bit order
GF_IF_HD inline uint32_t gf_if_crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ 0xedb88320u : b >> 1;
  }
  return p;
}

// x^(8 n) mod P
GF_IF_HD inline uint32_t gf_if_crc_shift(uint32_t n) {
  uint32_t p = 0x80000000u, sq = 0x00800000u;  // 1, x^8
  for (int i = 0; i < 32; i++) {
    if (n & 1u) p = gf_if_crc_mul(sq, p);
    sq = gf_if_crc_mul(sq, sq);
    n >>= 1;
  }
  return p;
}

// the CRC-32 of the whole text from its pieces' CRCs
GF_IF_HD inline uint32_t gf_if_crc_join(const uint32_t* pieces, uint32_t n) {
  const uint32_t op = gf_if_crc_shift(gf_if_crc_seg(n));
  uint32_t c = GF_IF_UNIFORM(pieces[0]);
  for (uint32_t k = 1; k < GF_IF_LANES; k++) c = gf_if_crc_mul(op, c) ^ GF_IF_UNIFORM(pieces[k]);
  return c;
}
