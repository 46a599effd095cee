/* gf_read_filter — quality filter and tail trimming of FASTQ records on the device: C ABI of libgfprep.so.
 *
 * GeneFuse expects reads that have been through a quality filter (its README names fastp and AfterQC); the reference
 * itself looks at a quality value only inside fast_merge (read.rs:232, :332-356).  This call is that step for records
 * that already sit in HBM between the FASTQ cut (gf_fastq_gather_device) and a scan: poly-G tails and low-quality
 * tails are cut off, and reads that are then too short, hold too many N or too many low bases are emptied.  It is a
 * feature outside the reference, and nothing calls it unless asked to.
 *
 * The predicate.  A read is its bases b[0..L) and its qualities q[0..L), one byte per base, the qualities at the
 * bases' offsets.  phred(j) = max(q[j] - 33, 0); a base is an N when it is not one of ACGTacgt.  In this order:
 *   1. poly-G tail: e1 = L; with poly_g_min > 0, t = the number of trailing bytes of b that are G or g (an exact run);
 *      t >= poly_g_min: e1 = L - t.
 *   2. tail cut by window: e2 = e1; with W = cut_tail_window > 0 and M = cut_tail_mean, e2 = the largest e with
 *      W <= e <= e1 and phred(e - W) + .. + phred(e - 1) >= W M; none (e1 < W too): e2 = 0.
 *   3. verdict on [0, e2), the first reason that applies: GF_PP_TOO_SHORT, e2 < length_required; GF_PP_TOO_MANY_N,
 *      more than n_base_limit N; GF_PP_LOW_QUALITY, 100 low > unqualified_percent e2, low the bases with
 *      phred < qualified_phred; else GF_PP_KEPT.
 *   4. pairs: when either mate has a reason, both are dropped; a mate without a reason of its own gets GF_PP_MATE_FAILED.
 *   5. a read longer than GF_MAX_READ_LEN passes as it is (GF_PP_KEPT, untrimmed; its mate's reason still drops it):
 *      the scans have their own answer for such reads.
 * The record count, order and indices do not change: a kept read is its first e2 bases and qualities, a dropped read a
 * record of length 0.
 *
 * A library of its own on top of libgfmatch.so (it uses gf_index_info_get of gfmatch.h to find the index's device).
 * Conventions are those of gfmatch.h: plain pointers and sizes, caller owns every buffer, GF_OK or a negative GF_ERR_*
 * code, with a message for the calling thread in gf_pp_last_error().  As in gfmatch.h the kernels load whole aligned
 * 16-byte chunks around a read: up to 15 bytes before its first and past its last byte are READ (never written, never
 * interpreted), which inside a device allocation is always addressable.
 */
#ifndef GF_READ_FILTER_H
#define GF_READ_FILTER_H

#include "gfmatch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GF_PP_KEPT 0
#define GF_PP_TOO_SHORT 1
#define GF_PP_TOO_MANY_N 2
#define GF_PP_LOW_QUALITY 3
#define GF_PP_MATE_FAILED 4
#define GF_PP_WINDOW_MAX 64
#define GF_PP_PHRED_MAX 93
#define GF_PP_TOTALS 8

/* The settings; gf_pp_filter_device refuses (GF_ERR_ARG) a negative value, cut_tail_window above GF_PP_WINDOW_MAX,
 * cut_tail_mean or qualified_phred above GF_PP_PHRED_MAX, unqualified_percent above 100, and poly_g_min or
 * length_required above GF_MAX_READ_LEN.  The defaults: 10, 0, 20, 15, 5, 15, 40. */
typedef struct gf_pp_settings {
  int32_t poly_g_min;          /* 0: no poly-G trimming */
  int32_t cut_tail_window;     /* 0: no tail cut; 1 .. 64: the window */
  int32_t cut_tail_mean;       /* the mean phred a tail window must reach */
  int32_t length_required;     /* the shortest read kept */
  int32_t n_base_limit;        /* the most N bases a kept read may have */
  int32_t qualified_phred;     /* a base below this is a low base */
  int32_t unqualified_percent; /* the share of low bases allowed */
} gf_pp_settings;

/* Device bytes gf_pp_filter_device needs as d_workspace for n records.  Non-decreasing in n. */
int64_t gf_pp_workspace_bytes(int64_t n);

/* The filter over n records, one asynchronous call queued on `stream` (a hipStream_t, NULL = default stream): no host
 * synchronisation, no allocation by this library and no copy between host and device, so that the call can be captured
 * into a graph.  Every pointer but `settings` is device memory on the index's device.
 *   d_l_bases / d_l_quals (uint8) and d_l_off (int64[n + 1], as gf_fastq_gather_device writes it): record i is bytes
 *     d_l_off[i] .. d_l_off[i + 1] of both; the offsets need not start at 0.  d_r_*: the mates, all three NULL for
 *     single-end input.
 *   d_workspace: gf_pp_workspace_bytes(n) bytes (GF_ERR_CAPACITY when smaller).
 * Output: the kept prefixes back to back in d_l_out_bases / d_l_out_quals (as many bytes as the records had:
 * trimming only shrinks), record i at d_l_out_off[i] .. d_l_out_off[i + 1] (int64[n + 1], from 0); the same for R with
 * the mates.  d_reasons (uint8[n], with mates uint8[2 n]: R1's, then R2's): GF_PP_* of every record.  d_totals
 * (int64[GF_PP_TOTALS]): [0] reads seen, [1] reads kept, [2] kept reads that were shortened, [3] bases removed from kept
 * reads, [4] dropped as too short, [5] for too many N, [6] for low quality, [7] for the mate only. */
int gf_pp_filter_device(const gf_index* idx, const gf_pp_settings* settings, const void* d_l_bases,
                        const void* d_l_quals, const void* d_l_off, const void* d_r_bases, const void* d_r_quals,
                        const void* d_r_off, int64_t n, void* d_workspace, int64_t workspace_bytes,
                        void* d_l_out_bases, void* d_l_out_quals, void* d_l_out_off, void* d_r_out_bases,
                        void* d_r_out_quals, void* d_r_out_off, void* d_reasons, void* d_totals, void* stream);

/* The message of the calling thread's last failed gf_pp_* call. */
const char* gf_pp_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* GF_READ_FILTER_H */
