// The FASTQ output of libgfwrite.so (include/gf_read_write.h), every formula that can go wrong by one written once:
// plain C++ that g++ compiles for the host (tests/cpp/test_read_write_core.cpp, under the sanitizers) and hipcc for the
// device (gf_rw_kernels.h).  The name line is gf_um_name_line's (gf_um_core.h), the chunks and the funnel shift are
// those of gf_dd_core.h.
//
//   a record     what one side of record i becomes: GF_RW_SEGS segments back to back — name head, tag, name tail, '\n',
//                bases, "\n+\n", qualities + '\n' — at the output positions start[0] = 0 .. start[7] = its size.  Four
//                of them are copied from memory (the text, the bases, the qualities), the tag is a few bytes of the
//                pre-cut records between ':' and '_', the rest are constants.
//   a piece      16 output bytes at a 16-byte aligned OUTPUT address.  With the record's first byte `a` bytes into its
//                piece 0, piece q holds the record's positions p = 16 q - a .. p + 15; it is full when all of them lie
//                in the record, and the first and the last piece of a record may be partial and shared with its
//                neighbours.  A piece is OR-ed together from the segments that overlap it: for a copied segment two
//                aligned 16-byte source chunks, funnel-shifted so that the source byte of position p comes first, and
//                masked to the overlap (gf_rw_take); chunks with no byte of the overlap are not loaded.
//   the walks    gf_rw_format_host below is the kernels' work by one thread, record after record and piece after piece,
//                over the same functions; its loads are bounded by the segment's own bytes.
#pragma once

#include <stdint.h>

#include "../../include/gf_read_write.h"
#include "gf_um_core.h"

#define GF_RW_HD GF_DD_HD
#define GF_RW_SEGS 7

// what gf_read_write.h accepts as settings
GF_RW_HD inline bool gf_rw_settings_ok(int32_t source, int32_t length, int32_t gather) {
  if (gather != GF_RW_WIDE && gather != GF_RW_BYTES) return false;
  if (source == GF_UM_NAME) return length == 0;
  return gf_um_inline_source(source) && length >= 1 && length <= GF_UM_MAX_LEN;
}

// the capacity bound: what a side's output can never pass
GF_RW_HD inline int64_t gf_rw_capacity(int64_t text_bytes, int64_t n) { return GF_RW_CAPACITY(text_bytes, n); }

// the name line of record i: text[s .. e); empty at the text's end when the text has no such line
GF_RW_HD inline void gf_rw_name_span(const int64_t* nl_pos, int64_t newlines, int64_t text_bytes, int64_t i, int64_t& s,
                                     int64_t& e) {
  if (!gf_um_name_line(nl_pos, newlines, text_bytes, i, s, e)) s = e = text_bytes;
}

// the length of the first token of the name line text[s .. e): up to the first space or tab, or the whole line
GF_RW_HD inline int64_t gf_rw_token_end(const uint8_t* text, int64_t s, int64_t e) {
  for (int64_t k = s; k < e; ++k)
    if (text[k] == ' ' || text[k] == '\t') return k - s;
  return e - s;
}

// whether a record (pair) with these lengths after all steps is written; len1 unused with sides == 1
GF_RW_HD inline bool gf_rw_written(int sides, int64_t len0, int64_t len1) { return len0 > 0 && (sides == 1 || len1 > 0); }

// the size of a written record
GF_RW_HD inline int64_t gf_rw_size(int64_t name_len, int64_t tag_len, int64_t len) {
  return name_len + tag_len + 2 * len + 5;
}

// The tag of a record: ':' + ua bytes at pre-cut side sa's from_a [+ '_' + ub bytes at side 1's from_b]; len 0: none.
struct gf_rw_tag {
  int32_t len, ua, ub;
  int sa;
  int64_t from_a, from_b;
};

// pre_from / pre_len: where the pre-cut records of the pair start and how long they are ([1] unused with sides == 1)
GF_RW_HD inline gf_rw_tag gf_rw_tag_of(int32_t source, int32_t length, int sides, const int64_t* pre_from,
                                       const int64_t* pre_len) {
  gf_rw_tag t{0, 0, 0, 0, 0, 0};
  if (!gf_um_inline_source(source)) return t;
  const bool two = sides == 2 && source == GF_UM_PER_READ;
  t.sa = sides == 2 && source == GF_UM_READ2 ? 1 : 0;
  t.ua = (int32_t)(pre_len[t.sa] < length ? pre_len[t.sa] : length);
  t.from_a = pre_from[t.sa];
  if (two) {
    t.ub = (int32_t)(pre_len[1] < length ? pre_len[1] : length);
    t.from_b = pre_from[1];
  }
  t.len = 1 + t.ua + (two ? 1 + t.ub : 0);
  return t;
}

struct gf_rw_record {
  int64_t start[GF_RW_SEGS + 1];  // the output position of every segment's first byte; start[GF_RW_SEGS]: the size
  int64_t name;                   // where the name line starts in the text
  int64_t from;                   // where the record starts in the bases and the qualities
  gf_rw_tag tag;
};

// the segment table of a written record: name line text[ns .. ne), its first token `tok` bytes (only looked at with a
// tag), `len` bases at `from`
GF_RW_HD inline gf_rw_record gf_rw_make_record(int64_t ns, int64_t ne, int64_t tok, const gf_rw_tag& tag, int64_t from,
                                               int64_t len) {
  gf_rw_record r;
  const int64_t name_len = ne - ns, head = tag.len ? tok : name_len;
  r.start[0] = 0;
  r.start[1] = head;
  r.start[2] = r.start[1] + tag.len;
  r.start[3] = r.start[2] + (name_len - head);
  r.start[4] = r.start[3] + 1;
  r.start[5] = r.start[4] + len;
  r.start[6] = r.start[5] + 3;
  r.start[7] = r.start[6] + len + 1;
  r.name = ns;
  r.from = from;
  r.tag = tag;
  return r;
}

// the segment that holds output position j (0 <= j < size)
GF_RW_HD inline int gf_rw_segment_of(const gf_rw_record& r, int64_t j) {
  int s = 0;
  while (s < GF_RW_SEGS - 1 && j >= r.start[s + 1]) ++s;
  return s;
}

// what a record is copied from: its side's text, bases and qualities, and the pre-cut bases of the tag's two parts
struct gf_rw_sources {
  const uint8_t* text;
  const uint8_t* bases;
  const uint8_t* quals;
  const uint8_t* pre_a;
  const uint8_t* pre_b;
};

// byte j (0 <= j < tag.len) of the tag
GF_RW_HD inline uint8_t gf_rw_tag_byte(const gf_rw_tag& t, const gf_rw_sources& S, int64_t j) {
  if (j == 0) return ':';
  if (j - 1 < t.ua) return S.pre_a[t.from_a + j - 1];
  if (j - 1 == t.ua) return '_';
  return S.pre_b[t.from_b + j - 2 - t.ua];
}

// output byte j (0 <= j < size) of a record: the plain gather
GF_RW_HD inline uint8_t gf_rw_byte(const gf_rw_record& r, const gf_rw_sources& S, int64_t j) {
  switch (gf_rw_segment_of(r, j)) {
    case 0: return S.text[r.name + j];
    case 1: return gf_rw_tag_byte(r.tag, S, j - r.start[1]);
    case 2: return S.text[r.name + j - r.tag.len];
    case 3: return '\n';
    case 4: return S.bases[r.from + j - r.start[4]];
    case 5: return j - r.start[5] == 1 ? '+' : '\n';
    default: return j < r.start[7] - 1 ? S.quals[r.from + j - r.start[6]] : '\n';
  }
}

// ---- pieces

// how many pieces a record of `size` bytes has whose first byte lies `a` bytes (0 .. 15) into its piece 0
GF_RW_HD inline int64_t gf_rw_pieces(int a, int64_t size) { return size > 0 ? (a + size + 15) >> 4 : 0; }

// the record's position of piece q's first byte: negative in a head piece
GF_RW_HD inline int64_t gf_rw_piece_pos(int a, int64_t q) { return 16 * q - a; }

// whether all 16 bytes of the piece at p belong to the record
GF_RW_HD inline bool gf_rw_piece_full(int64_t p, int64_t size) { return p >= 0 && p + 16 <= size; }

// the bytes [k_lo, k_hi) of the piece at p that belong to the record: what a head or tail piece stores, byte by byte
GF_RW_HD inline void gf_rw_piece_part(int64_t p, int64_t size, int& k_lo, int& k_hi) {
  k_lo = p < 0 ? (int)-p : 0;
  k_hi = size - p < 16 ? (int)(size - p) : 16;
}

// the bytes lo .. hi - 1 (clamped to 0 .. 8) of a 64-bit word as a mask
GF_RW_HD inline uint64_t gf_rw_bytes_mask(int lo, int hi) {
  lo = lo < 0 ? 0 : lo;
  hi = hi > 8 ? 8 : hi;
  if (lo >= hi) return 0;
  const uint64_t upto = hi == 8 ? ~0ull : (1ull << (8 * hi)) - 1ull;
  return upto & ~((1ull << (8 * lo)) - 1ull);
}

// byte k (0 .. 15) of a piece set (the piece holds 0 there)
GF_RW_HD inline void gf_rw_put(gf_dd_chunk& acc, int64_t k, uint8_t b) {
  if (k >= 0 && k < 16) acc.q[k >> 3] |= (uint64_t)b << (8 * (k & 7));
}

// The bytes of the copied segment [seg_start, seg_end) — its first source byte at src — that lie in the piece at p,
// OR-ed into acc.  load(address, first, last): the aligned 16-byte chunk at `address`, of which the caller needs only
// bytes of [first, last).
template <class Load>
GF_RW_HD inline void gf_rw_take(gf_dd_chunk& acc, const uint8_t* src, int64_t seg_start, int64_t seg_end, int64_t p,
                                Load load) {
  const int64_t lo = seg_start > p ? seg_start : p, hi = seg_end < p + 16 ? seg_end : p + 16;
  if (lo >= hi) return;
  const int k_lo = (int)(lo - p), k_hi = (int)(hi - p);
  // the source address of position p: in front of src in a piece the segment starts in
  const uintptr_t A = (uintptr_t)src + (uintptr_t)(p - seg_start);
  const int a = (int)(A & 15);
  const uintptr_t first = (uintptr_t)src, last = first + (uintptr_t)(seg_end - seg_start);
  // chunk 0 holds the piece's bytes 0 .. 15 - a, chunk 1 the bytes 16 - a .. 15
  const gf_dd_chunk c0 = k_lo < 16 - a ? load(A - a, first, last) : gf_dd_chunk{{0, 0}};
  const gf_dd_chunk c1 = k_hi > 16 - a ? load(A - a + 16, first, last) : gf_dd_chunk{{0, 0}};
  uint64_t w0, w1;
  gf_dd_piece_words(c0, c1, a, w0, w1);
  acc.q[0] |= w0 & gf_rw_bytes_mask(k_lo, k_hi);
  acc.q[1] |= w1 & gf_rw_bytes_mask(k_lo - 8, k_hi - 8);
}

// the piece at position p (-15 .. size - 1) of a record; bytes outside the record are 0
template <class Load>
GF_RW_HD inline gf_dd_chunk gf_rw_piece(const gf_rw_record& r, const gf_rw_sources& S, int64_t p, Load load) {
  gf_dd_chunk acc{{0, 0}};
  const int64_t len = r.start[5] - r.start[4];
  gf_rw_take(acc, S.text + r.name, r.start[0], r.start[1], p, load);
  if (r.tag.len) {
    const int64_t lo = r.start[1] > p ? r.start[1] : p, hi = r.start[2] < p + 16 ? r.start[2] : p + 16;
    for (int64_t j = lo; j < hi; ++j) gf_rw_put(acc, j - p, gf_rw_tag_byte(r.tag, S, j - r.start[1]));
  }
  gf_rw_take(acc, S.text + r.name + r.start[1], r.start[2], r.start[3], p, load);
  gf_rw_put(acc, r.start[3] - p, '\n');
  gf_rw_take(acc, S.bases + r.from, r.start[4], r.start[5], p, load);
  gf_rw_put(acc, r.start[5] - p, '\n');
  gf_rw_put(acc, r.start[5] + 1 - p, '+');
  gf_rw_put(acc, r.start[5] + 2 - p, '\n');
  gf_rw_take(acc, S.quals + r.from, r.start[6], r.start[6] + len, p, load);
  gf_rw_put(acc, r.start[7] - 1 - p, '\n');
  return acc;
}

// ---- a record of a call

// one side of a call, as the kernels take it
struct gf_rw_in {
  const uint8_t* text;
  int64_t text_bytes;
  const int64_t* nl_pos;
  int64_t newlines;
  const uint8_t* bases;
  const uint8_t* quals;
  const int64_t* off;
  const uint8_t* pre_bases;
  const int64_t* pre_off;
};

// Side `side` of record i of a call: its segment table and sources; returns its size, 0 when it is not written (r and S
// are then not set).  tok: the length of the name line's first token when the caller knows it, < 0: found here (only
// with a tag); lens: the pair's lengths after all steps.
GF_RW_HD inline int64_t gf_rw_describe(int32_t source, int32_t length, const gf_rw_in* in, int sides, int side,
                                       int64_t i, int64_t tok, gf_rw_record& r, gf_rw_sources& S, int64_t* lens) {
  int64_t from[2] = {0, 0};
  lens[0] = lens[1] = 0;
  for (int k = 0; k < sides; ++k) {
    from[k] = in[k].off[i];
    lens[k] = gf_dd_length(from[k], in[k].off[i + 1]);
  }
  if (!gf_rw_written(sides, lens[0], lens[1])) return 0;
  int64_t pre_from[2] = {0, 0}, pre_len[2] = {0, 0};
  if (gf_um_inline_source(source))
    for (int k = 0; k < sides; ++k) {
      pre_from[k] = in[k].pre_off[i];
      pre_len[k] = gf_dd_length(pre_from[k], in[k].pre_off[i + 1]);
    }
  const gf_rw_tag tag = gf_rw_tag_of(source, length, sides, pre_from, pre_len);
  int64_t ns, ne;
  gf_rw_name_span(in[side].nl_pos, in[side].newlines, in[side].text_bytes, i, ns, ne);
  if (tag.len && tok < 0) tok = gf_rw_token_end(in[side].text, ns, ne);
  r = gf_rw_make_record(ns, ne, tok, tag, from[side], lens[side]);
  S = gf_rw_sources{in[side].text, in[side].bases, in[side].quals, in[tag.sa].pre_bases, in[sides - 1].pre_bases};
  return r.start[GF_RW_SEGS];
}

// ---- the walks by one thread

// the host's load: a byte outside [first, last) is 0 and is not read
inline gf_dd_chunk gf_rw_load_host(uintptr_t address, uintptr_t first, uintptr_t last) {
  gf_dd_chunk v{{0, 0}};
  for (int k = 0; k < 16; ++k) {
    const uintptr_t p = address + k;
    if (p >= first && p < last) v.q[k >> 3] |= (uint64_t) * (const uint8_t*)p << (8 * (k & 7));
  }
  return v;
}

// one record written to `out`, its first output byte, as gf_rw_k_format writes it: full pieces in one store of 16
// bytes at a 16-byte aligned address, the partial ones byte by byte; gather GF_RW_BYTES: every byte on its own
inline void gf_rw_write_record_host(const gf_rw_record& r, const gf_rw_sources& S, uint8_t* out, int32_t gather) {
  const int64_t size = r.start[GF_RW_SEGS];
  if (gather == GF_RW_BYTES) {
    for (int64_t j = 0; j < size; ++j) out[j] = gf_rw_byte(r, S, j);
    return;
  }
  const int a = (int)((uintptr_t)out & 15);
  for (int64_t q = 0; q < gf_rw_pieces(a, size); ++q) {
    const int64_t p = gf_rw_piece_pos(a, q);
    const gf_dd_chunk v = gf_rw_piece(r, S, p, gf_rw_load_host);
    int k_lo = 0, k_hi = 16;
    if (!gf_rw_piece_full(p, size)) gf_rw_piece_part(p, size, k_lo, k_hi);
    for (int k = k_lo; k < k_hi; ++k) out[p + k] = (uint8_t)(v.q[k >> 3] >> (8 * (k & 7)));
  }
}

// The whole call by one thread: out_text[side] (out_cap[side] bytes), out_off[side] (int64[n + 1]), totals added into.
// A record that does not fit is left out of the text, as the kernel leaves it out.
inline void gf_rw_format_host(int32_t source, int32_t length, int32_t gather, const gf_rw_in* in, int sides, int64_t n,
                              uint8_t* const* out_text, const int64_t* out_cap, int64_t* const* out_off,
                              int64_t* totals) {
  int64_t at[2] = {0, 0};
  for (int64_t i = 0; i < n; ++i) {
    int64_t lens[2];
    bool written = false;
    for (int side = 0; side < sides; ++side) {
      gf_rw_record r;
      gf_rw_sources S;
      const int64_t size = gf_rw_describe(source, length, in, sides, side, i, -1, r, S, lens);
      out_off[side][i] = at[side];
      if (size > 0) {
        written = true;
        if (at[side] + size <= out_cap[side]) gf_rw_write_record_host(r, S, out_text[side] + at[side], gather);
        at[side] += size;
      }
    }
    if (written) {
      ++totals[0];
      totals[1] += lens[0] + lens[1];
    } else {
      ++totals[4];
    }
  }
  for (int side = 0; side < sides; ++side) {
    out_off[side][n] = at[side];
    totals[2 + side] += at[side];
  }
}
