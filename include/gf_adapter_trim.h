/* gf_adapter_trim — adapter trimming of FASTQ records on the device, by pair overlap and by sequence: C ABI of
 * libgfadapt.so.
 *
 * When a fragment is shorter than the reads, both mates read through the insert into the adapter.  fast_merge
 * (read.rs:313-440) only tries a tail of R1 against the head of rc(R2), an insert at least as long as the reads, so such
 * a pair never merges, and each mate carries an adapter tail into map_read.  This call cuts the records to the insert
 * while they sit in HBM between the FASTQ cut (gf_fastq_gather_device) and the read filter or a scan.  It is a feature
 * outside the reference, and nothing calls it unless asked to.
 *
 * The predicate.  Bases are compared case-folded.  x and y are complementary when {x, y} is {A, T} or {C, G}; a byte
 * that is not one of ACGTacgt is complementary to nothing.
 *   1. pair overlap (pairs, settings.overlap = 1).  R1 is a[0..L1), R2 is b[0..L2).  For an insert length I:
 *        lo = max(0, I - L2), hi = min(I, L1), ov(I) = hi - lo,
 *        d(I) = the number of i in [lo, hi) for which a[i] and b[I - 1 - i] are not complementary.
 *      I is accepted when ov(I) >= min_overlap, d(I) <= max_diff and 100 d(I) <= diff_percent ov(I).  The candidates
 *      are min_overlap <= I <= L1 + L2 - min_overlap, and I* is the LARGEST accepted I: the rule does not depend on a
 *      search order, and of the several accepted I of a tandem-repeat insert the largest cuts least.  With an I*, R1
 *      keeps min(L1, I*) bases and R2 keeps min(L2, I*), and step 2 is skipped for both mates.
 *   2. adapter sequence (single-end reads, and the mates of a pair without an I*).  A read's adapter A has nA bases,
 *      ACGT only, min_adapter <= nA <= GF_AT_ADAPTER_MAX; nA = 0: the read has none and this step does nothing.  R1 and
 *      single-end reads use adapter_r1, R2 uses adapter_r2.  For a read x[0..L) take the smallest p in
 *      [0, L - min_adapter] such that, with n = min(nA, L - p), x[p..p+n) differs from A[0..n) in at most floor(n / 10)
 *      positions; a byte of the read that is not one of ACGTacgt counts as a difference.  The read keeps p bases;
 *      p = 0, an adapter dimer, leaves a record of length 0.
 *   3. limits: a read of length 0, or longer than GF_AT_READ_MAX, passes as it is, and a pair with such a mate passes
 *      untouched on both sides.
 * The record count, order and indices do not change: a record is only ever replaced by a prefix of itself, bases and
 * qualities alike.
 *
 * A library of its own on top of libgfmatch.so (it uses gf_index_info_get of gfmatch.h to find the index's device).
 * Conventions are those of gfmatch.h: plain pointers and sizes, caller owns every buffer, GF_OK or a negative GF_ERR_*
 * code, with a message for the calling thread in gf_at_last_error().  As in gfmatch.h the kernels load whole aligned
 * 16-byte chunks around a read: up to 15 bytes before its first and past its last byte are READ (never written, never
 * interpreted), which inside a device allocation is always addressable.
 */
#ifndef GF_ADAPTER_TRIM_H
#define GF_ADAPTER_TRIM_H

#include "gfmatch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GF_AT_UNTOUCHED 0
#define GF_AT_BY_OVERLAP 1
#define GF_AT_BY_SEQUENCE 2
#define GF_AT_OVERLAP_CLEAN 3
#define GF_AT_READ_MAX 512
#define GF_AT_ADAPTER_MAX 64
#define GF_AT_TOTALS 6

/* The settings, 156 bytes.  gf_at_trim_device refuses (GF_ERR_ARG): overlap other than 0 or 1; min_overlap outside
 * 8 .. GF_AT_READ_MAX; a negative max_diff; diff_percent outside 0 .. 100; min_adapter outside 4 .. GF_AT_ADAPTER_MAX;
 * an adapter length that is neither 0 nor within min_adapter .. GF_AT_ADAPTER_MAX; an adapter with a byte that is not
 * one of ACGT; overlap = 0 with no adapter (nothing to do); single-end input without adapter_r1.
 * The defaults: 1, 30, 5, 20, 10, 0, 0. */
typedef struct gf_at_settings {
  int32_t overlap;        /* 1: step 1 for pairs; 0: the sequence step only */
  int32_t min_overlap;    /* the fewest positions an accepted insert compares */
  int32_t max_diff;       /* the most differences of an accepted insert */
  int32_t diff_percent;   /* the share of differences of an accepted insert */
  int32_t min_adapter;    /* the fewest adapter bases looked for at a read's end */
  int32_t adapter_r1_len; /* 0: none */
  int32_t adapter_r2_len; /* 0: none */
  uint8_t adapter_r1[64];
  uint8_t adapter_r2[64];
} gf_at_settings;

/* Device bytes gf_at_trim_device needs as d_workspace for n records.  Non-decreasing in n; 0 for n < 0. */
int64_t gf_at_workspace_bytes(int64_t n);

/* The trimming of n records, one asynchronous call queued on `stream` (a hipStream_t, NULL = default stream): no host
 * synchronisation, no allocation by this library and no copy between host and device, so that the call can be captured
 * into a graph.  The contract is that of gf_pp_filter_device (gf_read_filter.h), so that the two calls chain.  Every
 * pointer but `settings` is device memory on the index's device.
 *   d_l_bases / d_l_quals (uint8) and d_l_off (int64[n + 1], as gf_fastq_gather_device writes it): record i is bytes
 *     d_l_off[i] .. d_l_off[i + 1] of both; the offsets need not start at 0.  d_r_*: the mates, all three NULL for
 *     single-end input.
 *   d_workspace: gf_at_workspace_bytes(n) bytes (GF_ERR_CAPACITY when smaller).
 * Output: the kept prefixes back to back in d_l_out_bases / d_l_out_quals (as many bytes as the records had:
 * trimming only shrinks), record i at d_l_out_off[i] .. d_l_out_off[i + 1] (int64[n + 1], from 0); the same for R with
 * the mates.  d_how (uint8[n], with mates uint8[2 n]: R1's, then R2's): GF_AT_UNTOUCHED, nothing found;
 * GF_AT_BY_OVERLAP, cut by step 1; GF_AT_BY_SEQUENCE, cut by step 2; GF_AT_OVERLAP_CLEAN, the pair has an I* and it is
 * at least this read's length.  d_totals (int64[GF_AT_TOTALS]): [0] reads seen, [1] reads cut, [2] bases removed,
 * [3] reads cut by overlap, [4] reads cut by sequence, [5] pairs with an I*. */
int gf_at_trim_device(const gf_index* idx, const gf_at_settings* settings, const void* d_l_bases,
                      const void* d_l_quals, const void* d_l_off, const void* d_r_bases, const void* d_r_quals,
                      const void* d_r_off, int64_t n, void* d_workspace, int64_t workspace_bytes,
                      void* d_l_out_bases, void* d_l_out_quals, void* d_l_out_off, void* d_r_out_bases,
                      void* d_r_out_quals, void* d_r_out_off, void* d_how, void* d_totals, void* stream);

/* The message of the calling thread's last failed gf_at_* call. */
const char* gf_at_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* GF_ADAPTER_TRIM_H */
