/* gf_overlap_correct — bases inside the overlap of a pair corrected from the mate, on the device: C ABI of
 * libgfcorrect.so.
 *
 * Where the mates of a pair read the same bases of the fragment, a base is observed twice.  When the two observations
 * disagree and one of them is a confident call while the other is a poor one, the poor one is a miscall that the mate
 * already contradicts.  fast_merge tolerates at most two low-quality mismatches in the overlap, the duplicate removal
 * keys on the exact bases, and the cleaned reads are handed to an aligner as they are: each of them carries such
 * miscalls on.  This call rewrites them while the records sit in HBM between the FASTQ cut (gf_fastq_gather_device)
 * and the adapter trimming.  It is a feature outside the reference, and nothing calls it unless asked to.
 *
 * The predicate.  Pairs only: R1 is a[0..L1) with the qualities qa, R2 is b[0..L2) with the qualities qb.
 * phred(q) = max(q - 33, 0), as in gf_read_filter.h.  "Complementary" and "case-folded" are those of
 * gf_adapter_trim.h: bases are compared case-folded, x and y are complementary when {x, y} is {A, T} or {C, G}, and a
 * byte that is not one of ACGTacgt is complementary to nothing.
 *   1. I*.  Exactly step 1 of gf_adapter_trim.h with this call's min_overlap, max_diff and diff_percent: for an insert
 *      length I, lo = max(0, I - L2), hi = min(I, L1), ov(I) = hi - lo, d(I) = the number of i in [lo, hi) for which
 *      a[i] and b[I - 1 - i] are not complementary; I is accepted when ov(I) >= min_overlap, d(I) <= max_diff and
 *      100 d(I) <= diff_percent ov(I); I* is the LARGEST accepted I among min_overlap <= I <= L1 + L2 - min_overlap.
 *      A pair with a mate of length 0, or longer than GF_AT_READ_MAX, passes untouched, and so does a pair without
 *      an I*.
 *   2. the correction at I*.  With lo = max(0, I* - L2) and hi = min(I*, L1), every i in [lo, hi) faces
 *      j = I* - 1 - i.  A difference is a position where a[i] and b[j] are not complementary; there are
 *      d(I*) <= max_diff of them.  At a difference:
 *        R2 is corrected when a[i] is one of ACGTacgt, phred(qa[i]) >= good_phred and phred(qb[j]) <= bad_phred:
 *          b[j] becomes the upper-case complement of a[i], and qb[j] becomes qa[i];
 *        otherwise R1 is corrected when b[j] is one of ACGTacgt, phred(qb[j]) >= good_phred and
 *          phred(qa[i]) <= bad_phred: a[i] becomes the upper-case complement of b[j], and qa[i] becomes qb[j];
 *        otherwise the difference is left standing.
 *      So a low-quality N (or any other byte) that faces a good base is corrected: what is overwritten need not be a
 *      base.  A byte that is not one of ACGTacgt is never a source, whatever its quality: an N of good quality that
 *      faces a poor base corrects nothing.  A lower-case source is written as its upper-case complement.  Two good
 *      calls that disagree, and two poor ones, are left standing: bad_phred < good_phred, so at most one of the two
 *      rules holds.  Every byte belongs to at most one (i, j), so the result does not depend on an order.
 * Lengths, offsets, the record count and the order do not change: bytes are replaced where they lie.
 *
 * A library of its own on top of libgfmatch.so (it uses gf_index_info_get of gfmatch.h to find the index's device).
 * Conventions are those of gfmatch.h: plain pointers and sizes, caller owns every buffer, GF_OK or a negative GF_ERR_*
 * code, with a message for the calling thread in gf_oc_last_error().  As in gfmatch.h the kernel loads whole aligned
 * 16-byte chunks around a read: up to 15 bytes before its first and past its last byte are READ (never interpreted),
 * which inside a device allocation is always addressable.  It WRITES single bytes of the records only.
 */
#ifndef GF_OVERLAP_CORRECT_H
#define GF_OVERLAP_CORRECT_H

#include "gf_adapter_trim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GF_OC_TOTALS 6
#define GF_OC_PHRED_MAX 93

/* The settings, 20 bytes.  gf_oc_correct_device refuses (GF_ERR_ARG, "settings: ..."): min_overlap outside
 * 8 .. GF_AT_READ_MAX; a negative max_diff; diff_percent outside 0 .. 100; good_phred or bad_phred outside
 * 0 .. GF_OC_PHRED_MAX; bad_phred not below good_phred.  The defaults: 30, 5, 20, 30, 15 (the last two are fast_merge's
 * '?' and '0'). */
typedef struct gf_oc_settings {
  int32_t min_overlap;  /* the fewest positions an accepted insert compares */
  int32_t max_diff;     /* the most differences of an accepted insert */
  int32_t diff_percent; /* the share of differences of an accepted insert */
  int32_t good_phred;   /* a source's phred is at least this */
  int32_t bad_phred;    /* a corrected base's phred is at most this */
} gf_oc_settings;

/* The correction of n pairs IN PLACE, one asynchronous call queued on `stream` (a hipStream_t, NULL = default stream):
 * no host synchronisation, no allocation by this library and no copy between host and device, so that the call can be
 * captured into a graph.  Every pointer but `settings` is device memory on the index's device.
 *   d_l_bases / d_l_quals (uint8) and d_l_off (int64[n + 1], as gf_fastq_gather_device writes it): R1 of pair i is
 *     bytes d_l_off[i] .. d_l_off[i + 1] of both; the offsets need not start at 0.  d_r_*: the mates, R2.  The call is
 *     for pairs: without mates it is GF_ERR_ARG.
 *   d_insert (int32[n], may be NULL): I* of every pair, -1 without one.
 *   d_fixed (int32[2 n], may be NULL): the bases corrected in each R1, then in each R2.
 *   d_totals (int64[GF_OC_TOTALS]): [0] pairs seen, [1] pairs with an I*, [2] pairs with at least one difference at
 *     I*, [3] reads corrected, [4] bases corrected, [5] differences left standing.
 * Host memory behind the offsets is GF_ERR_NO_DEVICE: there is no CPU fallback. */
int gf_oc_correct_device(const gf_index* idx, const gf_oc_settings* settings, void* d_l_bases, void* d_l_quals,
                         const void* d_l_off, void* d_r_bases, void* d_r_quals, const void* d_r_off, int64_t n,
                         void* d_insert, void* d_fixed, void* d_totals, void* stream);

/* The message of the calling thread's last failed gf_oc_* call. */
const char* gf_oc_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* GF_OVERLAP_CORRECT_H */
