/* gf_single_end — the single-end scan of GeneFuse on the device: C ABI of libgfse.so.
 *
 * SingleEndScanner::scan_single_end (src/core/sescanner.rs:183-205) for a batch of n records resident in HBM, in
 * the layout gf_fastq_gather_device writes (bases and qualities back to back at the same offsets, int64[n+1]):
 *   every read is mapped (Indexer::map_read); a read that gives two segments (`mapable`, fusion_mapper.rs:107-115)
 *   in the required direction (:118-123) is a hit; one that gives two segments in the wrong direction is searched
 *   again as its reverse complement (SequenceRead::reverse_complement: complement to upper case, anything but
 *   ACGTacgt becomes N, qualities reversed), which is a hit when ITS two segments are in the required direction.
 *
 * A library of its own on top of libgfmatch.so: it drives the mapping only through the public ABI of gfmatch.h
 * (gf_map_reads_device), and adds the classification, reverse-complement and compaction kernels.  Conventions are
 * those of gfmatch.h: plain pointers and sizes, caller owns every buffer, GF_OK or a negative GF_ERR_* code, with a
 * message for the calling thread in gf_se_last_error().
 */
#ifndef GF_SINGLE_END_H
#define GF_SINGLE_END_H

#include "gfmatch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The default number of reverse-complement retry slots for a batch of n reads (retry_cap <= 0 selects it). */
int64_t gf_se_retry_capacity(int64_t n);

/* Device bytes gf_se_scan_device needs as d_workspace for n reads of at most max_read_len bases with retry_cap
 * retry slots (<= 0: gf_se_retry_capacity(n)).  Non-decreasing in n and in a positive retry_cap. */
int64_t gf_se_workspace_bytes(int64_t n, int32_t max_read_len, int64_t retry_cap);

/* The scan of n single-end reads, one asynchronous call queued on `stream` (a hipStream_t, NULL = default stream):
 * no host synchronisation, no allocation by this library and no copy between host and device, so that the call
 * can be captured into a graph.  Every pointer is device memory on the index's device.
 *   d_bases / d_quals (uint8) and d_offsets (int64[n+1]): read r is bases[offsets[r] .. offsets[r+1]), its qualities
 *     at the same offsets; n_bytes = bytes in the base buffer.  max_read_len bounds the read lengths
 *     (<= GF_MAX_READ_LEN); a longer read is counted in d_totals[5] and never a hit.
 *   d_gene_reversed: uint8[n_genes], Fusion::is_reversed() per gene (gene.rs:98-107); NULL = all false.
 *   retry_cap: reverse-complement retry slots (<= 0: gf_se_retry_capacity(n); at most n are used).
 *   d_workspace: gf_se_workspace_bytes(n, max_read_len, retry_cap) bytes (GF_ERR_CAPACITY when smaller).
 * Output, in read order, in the format of gf_scan_pairs_device: one gf_pair_hit per hit with pair_id =
 * read_id_base + r, source = 1, flags = 3 when the hit is on the reverse complement (else 0), merge_diff = 0, and the
 * matched read's bases and qualities (the reverse complement's, qualities reversed) at seq_offset of d_hit_bases /
 * d_hit_quals.  A record is written while it fits hits_cap, a read's bytes only when all of them fit hit_bytes_cap.
 * d_totals (int64[8]): [0] hits, [1] bytes of their reads, [2] 0, [3] reads searched again reversed, [4] overflow
 * bits — 1: more retries than retry_cap (the retry pass was emptied: run again with retry_cap = n), 2: more hits or
 * bytes than the output capacities ([0], [1] say how many) — [5] reads whose count came back GF_COUNT_TOO_LONG,
 * [6], [7] 0. */
int gf_se_scan_device(const gf_index* idx, const void* d_bases, const void* d_quals, const void* d_offsets,
                      int64_t n_bytes, int64_t n, int32_t max_read_len, const void* d_gene_reversed, int32_t n_genes,
                      int64_t read_id_base, int64_t retry_cap, void* d_workspace, int64_t workspace_bytes, void* d_hits,
                      int64_t hits_cap, void* d_hit_bases, void* d_hit_quals, int64_t hit_bytes_cap, void* d_totals,
                      void* stream);

/* The message of the calling thread's last failed gf_se_* call. */
const char* gf_se_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* GF_SINGLE_END_H */
