/* gf_read_qc — per-cycle quality and base-content tables and the insert-size histogram of FASTQ records on the device:
 * C ABI of libgfqc.so.
 *
 * With the read filter (gf_read_filter.h) and the adapter trimming (gf_adapter_trim.h) on the device a pipeline needs no
 * fastp in front of a scan, and so it has no QC report: reads and bases before and after filtering, Q20 / Q30 rates, GC
 * content, the per-cycle curves, the insert sizes.  These calls take the numbers all of that is derived from while the
 * records sit in HBM between the FASTQ cut (gf_fastq_gather_device) and a scan.  They read, and write nothing but their
 * tables.  A feature outside the reference, and nothing calls it unless asked to.
 *
 * The definitions, shared with gf_read_filter.h.  A read is its bases b[0..L) and its qualities q[0..L), one byte per
 * base, the qualities at the bases' offsets.  phred(j) = max(q[j] - 33, 0).  A base is one of ACGTacgt, either case
 * counting as the letter; any other byte is an N.  A record whose offsets run backwards has length 0.  The offsets need
 * not start at 0.
 *
 * The table of one side, int64[GF_QC_SIDE_WORDS], with C = GF_QC_CYCLES = 512:
 *   length_hist[C + 1]   words 0 .. C: a record of length L counts in entry min(L, C).  Entry 0 holds the records of
 *                        length 0, which are not reads.
 *   cycle[C + 1][8]      words C + 1 + 8 c + column: row c < C holds the bases at position c of their read, row C every
 *                        base at a position >= C.  The columns (GF_QC_COL_*): A, C, G, T, N, qual_sum (the sum of
 *                        phred), q20 (phred >= 20), q30 (phred >= 30).
 * A record of any length is counted in full: there is no GF_MAX_READ_LEN exemption here.  Reads, bases, GC, rates and
 * mean lengths are sums over these words, taken on the host.
 *
 * The insert histogram, int64[GF_QC_INSERT_WORDS].  For a pair whose mates both have 1 .. GF_AT_READ_MAX (512) bases, I*
 * is the largest insert I in 30 .. L1 + L2 - 30 that the overlap predicate of gf_adapter_trim.h (step 1) accepts with
 * that header's defaults: ov(I) >= 30, d(I) <= 5 and 100 d(I) <= 20 ov(I).  The settings are fixed here, whatever
 * trimming a scan uses.  hist[I*] += 1; with no accepted insert hist[0] += 1; a pair with a mate of length 0 or above
 * 512 counts in hist[GF_QC_INSERT_UNMEASURED] (1025).  Entries 1 .. 29 and 995 .. 1024 stay 0.
 *
 * Both calls ADD into their table and never zero it: the caller zeroes it once, and chunks accumulate in HBM.  Every
 * number is an exact integer sum, so the tables do not depend on the order of the work.
 *
 * A library of its own on top of libgfmatch.so (it uses gf_index_info_get of gfmatch.h to find the index's device).
 * Conventions are those of gfmatch.h: plain pointers and sizes, caller owns every buffer, GF_OK or a negative GF_ERR_*
 * code, with a message for the calling thread in gf_qc_last_error().  As in gf_read_filter.h the kernels may load whole
 * aligned 16-byte chunks around a read: up to 15 bytes before its first and past its last byte may be READ (never
 * written, never interpreted), which inside a device allocation is always addressable.
 */
#ifndef GF_READ_QC_H
#define GF_READ_QC_H

#include "gfmatch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GF_QC_CYCLES 512
#define GF_QC_COLUMNS 8
#define GF_QC_SIDE_WORDS 4617 /* (GF_QC_CYCLES + 1) + (GF_QC_CYCLES + 1) * GF_QC_COLUMNS */
#define GF_QC_INSERT_WORDS 1026
#define GF_QC_INSERT_UNMEASURED 1025
#define GF_QC_INSERT_MIN 30
#define GF_QC_COL_A 0
#define GF_QC_COL_C 1
#define GF_QC_COL_G 2
#define GF_QC_COL_T 3
#define GF_QC_COL_N 4
#define GF_QC_COL_QUAL_SUM 5
#define GF_QC_COL_Q20 6
#define GF_QC_COL_Q30 7

/* The table of one side's n records, added into d_table (int64[GF_QC_SIDE_WORDS]): one asynchronous call queued on
 * `stream` (a hipStream_t, NULL = default stream): no host synchronisation, no allocation by this library and no copy
 * between host and device, so that the call can be captured into a graph.  Every pointer is device memory on the
 * index's device.
 *   d_bases / d_quals (uint8) and d_off (int64[n + 1], as gf_fastq_gather_device writes it): record i is bytes
 *     d_off[i] .. d_off[i + 1] of both.
 * n = 0 is GF_OK and queues nothing.  GF_ERR_ARG: a NULL index, table or offsets, NULL bases or qualities with
 * records, n negative or above 2^38. */
int gf_qc_stats_device(const gf_index* idx, const void* d_bases, const void* d_quals, const void* d_off, int64_t n,
                       void* d_table, void* stream);

/* The insert lengths of n pairs, added into d_hist (int64[GF_QC_INSERT_WORDS]); the contract is that of
 * gf_qc_stats_device.  d_l_bases / d_l_off: R1's records, d_r_bases / d_r_off: their mates, record by record. */
int gf_qc_insert_device(const gf_index* idx, const void* d_l_bases, const void* d_l_off, const void* d_r_bases,
                        const void* d_r_off, int64_t n, void* d_hist, void* stream);

/* The message of the calling thread's last failed gf_qc_* call. */
const char* gf_qc_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* GF_READ_QC_H */
