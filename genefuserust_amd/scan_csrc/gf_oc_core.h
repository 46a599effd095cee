// The overlap correction of libgfcorrect.so (include/gf_overlap_correct.h), the arithmetic written once: plain C++ that
// g++ compiles for the host (tests/cpp/test_overlap_correct_core.cpp, under the sanitizers) and hipcc for the device
// (gf_oc_kernels.h).
//
// The search for I* is gf_at_core.h's, included as it is: the planes of a forwards and of rc(b), an insert a funnel
// shift, rounds of G candidates from the largest downwards.  What is new happens at I*:
//
//   a difference word   the 32 positions 32 w .. 32 w + 31 of a at the insert I: the very expression gf_at_try_insert
//                       counts, kept as a mask.  Bit k set: a[32 w + k] and b[I - 1 - 32 w - k] are not complementary,
//                       and 32 w + k lies in [lo, hi).
//   a decision          one difference, its four bytes: which mate is rewritten, if any.
//   a pair              gf_oc_correct_pair below is the kernel's walk by one thread: the planes, I*, then word after
//                       word, bit after bit, single bytes read and single bytes written.
//
// Nothing outside the chunks 0 .. (a + L - 1) / 16 of a read is loaded, nothing but bytes of the two records is written.
#pragma once

#include "../../include/gf_overlap_correct.h"
#include "gf_at_core.h"

#define GF_OC_LEFT 0    // the difference is left standing
#define GF_OC_FIX_R1 1  // a[i], qa[i] are rewritten from b[j], qb[j]
#define GF_OC_FIX_R2 2  // b[j], qb[j] are rewritten from a[i], qa[i]

// NULL, or what is wrong with the settings (include/gf_overlap_correct.h)
GF_AT_HD inline const char* gf_oc_settings_error(const gf_oc_settings& s) {
  if (s.min_overlap < 8 || s.min_overlap > GF_AT_READ_MAX) return "min_overlap outside 8 .. 512";
  if (s.max_diff < 0) return "a negative max_diff";
  if (s.diff_percent < 0 || s.diff_percent > 100) return "diff_percent outside 0 .. 100";
  if (s.good_phred < 0 || s.good_phred > GF_OC_PHRED_MAX) return "good_phred outside 0 .. 93";
  if (s.bad_phred < 0 || s.bad_phred > GF_OC_PHRED_MAX) return "bad_phred outside 0 .. 93";
  if (s.bad_phred >= s.good_phred) return "bad_phred not below good_phred";
  return nullptr;
}

// the settings gf_at_core.h's search takes: the overlap step alone, no adapter
GF_AT_HD inline gf_at_settings gf_oc_search_settings(const gf_oc_settings& s) {
  gf_at_settings t = {};
  t.overlap = 1;
  t.min_overlap = s.min_overlap;
  t.max_diff = s.max_diff;
  t.diff_percent = s.diff_percent;
  t.min_adapter = 10;
  return t;
}

// The differences among a's positions 32 w .. 32 w + 31 at the insert I, (lo >> 5) <= w <= ((hi - 1) >> 5).
// A: the planes of a, R: those of rc(b).  The sum of its popcounts over those w is gf_at_try_insert's d.
GF_AT_HD inline uint32_t gf_oc_diff_word(const uint32_t* A, const uint32_t* R, int32_t L1, int32_t L2, int32_t I,
                                         int32_t w) {
  const int32_t shift = L2 - I;
  const int32_t lo = I > L2 ? I - L2 : 0, hi = I < L1 ? I : L1;
  const int32_t t = 32 * w + shift + 32;  // (>= 1: the word holds a position of [lo, hi))
  const int q = t >> 5, r = t & 31;
  const uint32_t diff = (A[w + 1] ^ gf_at_funnel(R[q], R[q + 1], r)) |
                        (A[GF_AT_PLANE + w + 1] ^ gf_at_funnel(R[GF_AT_PLANE + q], R[GF_AT_PLANE + q + 1], r)) |
                        A[2 * GF_AT_PLANE + w + 1] | gf_at_funnel(R[2 * GF_AT_PLANE + q], R[2 * GF_AT_PLANE + q + 1], r);
  return diff & gf_at_range(32 * w, lo, hi);
}

GF_AT_HD inline bool gf_oc_is_base(uint8_t c) {
  c |= 0x20;
  return c == 'a' || c == 'c' || c == 'g' || c == 't';
}

// the upper-case complement of one of ACGTacgt
GF_AT_HD inline uint8_t gf_oc_complement(uint8_t c) {
  c |= 0x20;
  return c == 'a' ? 'T' : c == 'c' ? 'G' : c == 'g' ? 'C' : 'A';
}

// one difference: a base and its quality of R1, those of R2 it faces
GF_AT_HD inline int gf_oc_decide(uint8_t a, uint8_t qa, uint8_t b, uint8_t qb, const gf_oc_settings& s) {
  const int32_t pa = (int32_t)gf_pp_phred(qa), pb = (int32_t)gf_pp_phred(qb);
  if (gf_oc_is_base(a) && pa >= s.good_phred && pb <= s.bad_phred) return GF_OC_FIX_R2;
  if (gf_oc_is_base(b) && pb >= s.good_phred && pa <= s.bad_phred) return GF_OC_FIX_R1;
  return GF_OC_LEFT;
}

// what one difference word of a pair came to
struct gf_oc_counts {
  int32_t fixed[2];  // bases corrected in R1, in R2
  int32_t left;      // differences left standing
};

// The differences `mask` of word w at the insert I, one after the other: the four bytes read, two of them written.
// a / qa / b / qb: the first byte of the records' bases and qualities.
GF_AT_HD inline void gf_oc_correct_word(uint32_t mask, int32_t w, int32_t I, uint8_t* a, uint8_t* qa, uint8_t* b,
                                        uint8_t* qb, const gf_oc_settings& s, gf_oc_counts& c) {
  while (mask) {
    const int k = __builtin_ctz(mask);
    mask &= mask - 1;
    const int32_t i = 32 * w + k, j = I - 1 - i;
    const uint8_t xa = a[i], xqa = qa[i], xb = b[j], xqb = qb[j];
    const int what = gf_oc_decide(xa, xqa, xb, xqb, s);
    if (what == GF_OC_FIX_R2) {
      b[j] = gf_oc_complement(xa);
      qb[j] = xqa;
      ++c.fixed[1];
    } else if (what == GF_OC_FIX_R1) {
      a[i] = gf_oc_complement(xb);
      qa[i] = xqb;
      ++c.fixed[0];
    } else {
      ++c.left;
    }
  }
}

// ---- a pair, by one thread: the walk of gf_oc_k_correct, lane after lane ----------------------------------------------

// load_l(c) / load_r(c): chunk c of the mates' bases; al / ar: how far into its chunk 0 each mate's first byte lies;
// a / qa / b / qb: the records' first bytes.  Returns I*, -1 without one (nothing is written then); `c`: the counts.
template <int G, class LoadL, class LoadR>
GF_AT_HD inline int32_t gf_oc_correct_pair(LoadL load_l, int al, int64_t len_l, LoadR load_r, int ar, int64_t len_r,
                                           uint8_t* a, uint8_t* qa, uint8_t* b, uint8_t* qb, const gf_oc_settings& s,
                                           gf_oc_counts& c) {
  c.fixed[0] = c.fixed[1] = c.left = 0;
  if (gf_at_passes(len_l) || gf_at_passes(len_r)) return -1;
  const int32_t L1 = (int32_t)len_l, L2 = (int32_t)len_r;
  const gf_at_settings t = gf_oc_search_settings(s);
  uint32_t A[GF_AT_READ_WORDS], R[GF_AT_READ_WORDS];
  gf_at_pack_read(load_l, al, L1, false, A);
  gf_at_pack_read(load_r, ar, L2, true, R);
  const int32_t I = gf_at_find_insert<G>(A, R, L1, L2, t);
  if (I < 0) return -1;
  const int32_t lo = I > L2 ? I - L2 : 0, hi = I < L1 ? I : L1;
  for (int32_t w = lo >> 5; w <= (hi - 1) >> 5; ++w)
    gf_oc_correct_word(gf_oc_diff_word(A, R, L1, L2, I, w), w, I, a, qa, b, qb, s, c);
  return I;
}
