/* gf_multi_csv — the paired-end scan of GeneFuse's multi-CSV mode on the device: C ABI of libgfmcsv.so.
 *
 * Multi-CSV mode (FusionScan::scan_per_fusion_csv, src/core/fusion_scan.rs:62-188) reads the FASTQ records once and
 * scans them against one index per fusion CSV.  PairEndScanner::scan_pair_end (src/core/pescanner.rs:427-518) has a
 * half that does not depend on the CSV and a half that does, and this library splits it there:
 *
 *   gf_mc_pairs_prepare_device   ONCE per read set: fast_merge of every pair (read.rs:313-440), the reads a scan will
 *                                map gathered into two contiguous lists (R1, R2 of the pairs that did not merge; the
 *                                merged reads), and those lists in the packed form of gf_pack_bases_device
 *   gf_mc_pairs_scan_device      ONCE per index: the two lists mapped from the packed form, the direction gate
 *                                (fusion_mapper.rs:107-123), the reverse-complement retries (read.rs:243-261), a mapping
 *                                pass over those, and the ordered compaction into exactly the output of
 *                                gf_scan_pairs_device
 *
 * A library of its own on top of libgfmatch.so: it drives the merge, the packing and the mapping only through the
 * public ABI of gfmatch.h and adds the gather, classification, reverse-complement and compaction kernels
 * (gf_mc_k_*).  Conventions are those of gfmatch.h and gf_single_end.h: plain pointers and sizes, the caller owns
 * every buffer (prepared buffer and workspace included), no allocation by this library, no host synchronisation and
 * no copy between host and device inside a call, everything queued on the caller's hipStream_t (NULL = default
 * stream), GF_OK or a negative GF_ERR_* code with a message for the calling thread in gf_mc_last_error().  Argument
 * errors are reported before any device is touched.
 */
#ifndef GF_MULTI_CSV_H
#define GF_MULTI_CSV_H

#include "gfmatch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device bytes of the prepared buffer of n pairs whose R1 / R2 base buffers hold l_bytes / r_bytes bytes, reads of at
 * most max_read_len bases.  Non-decreasing in n, l_bytes and r_bytes; 0 for a negative argument.  It holds, per
 * pair, the merged length, merged_diff, the pair's place in its list and the merged read's position; the offsets of
 * both lists; the reads' bases (l_bytes + r_bytes: a merged read is shorter than its pair) and the merged reads'
 * qualities; the packed form of the bases (6 bytes per 16); and the tile sums of the gather. */
int64_t gf_mc_prepared_bytes(int64_t n, int64_t l_bytes, int64_t r_bytes, int32_t max_read_len);

/* The CSV-independent half for n pairs resident in HBM, in the layout gf_fastq_gather_device writes (R1 = l_*, R2 =
 * r_*, R2 as read from its file; offsets int64[n+1], the same for bases and qualities; l_bytes / r_bytes = bytes in
 * the base buffers).  `idx` only names the device (the merge does not look at the table): d_prepared stays valid
 * after that index is freed and is scanned with any index on the same device.  max_read_len bounds the read lengths
 * (2 * max_read_len <= GF_MAX_READ_LEN).  d_prepared: gf_mc_prepared_bytes(n, l_bytes, r_bytes, max_read_len) bytes
 * (prepared_bytes says how many there are: GF_ERR_CAPACITY when fewer). */
int gf_mc_pairs_prepare_device(const gf_index* idx, const void* d_l_bases, const void* d_l_quals, const void* d_l_offsets,
                               int64_t l_bytes, const void* d_r_bases, const void* d_r_quals, const void* d_r_offsets,
                               int64_t r_bytes, int64_t n, int32_t max_read_len, void* d_prepared, int64_t prepared_bytes,
                               void* stream);

/* The default number of reverse-complement retry slots for n pairs (retry_cap <= 0 selects it).  The retry pass maps
 * every slot, the number of retries being on the device, so the default is small: n / 32 (real panels retry a few
 * reads per ten thousand), 4096 at least.  gf_scan_pairs_device, which maps exactly the retries there are, has n / 4. */
int64_t gf_mc_retry_capacity(int64_t n);

/* Device bytes gf_mc_pairs_scan_device needs as d_workspace for n pairs of reads of at most max_read_len bases with
 * retry_cap retry slots (<= 0: gf_mc_retry_capacity(n); at most 3 n are used).  Non-decreasing in n and in a positive
 * retry_cap; 0 for a negative n or max_read_len. */
int64_t gf_mc_scan_workspace_bytes(int64_t n, int32_t max_read_len, int64_t retry_cap);

/* The CSV-dependent half: the pairs of d_prepared (as gf_mc_pairs_prepare_device left it for the same n, l_bytes,
 * r_bytes, max_read_len and R1 / R2 buffers, on this stream or synchronised with it) against `idx`.
 *   d_gene_reversed: uint8[n_genes], Fusion::is_reversed() per gene (gene.rs:98-107); NULL = all false.
 *   retry_cap: reverse-complement retry slots (<= 0: gf_mc_retry_capacity(n); at most 3 n are used).
 *   d_workspace: gf_mc_scan_workspace_bytes(n, max_read_len, retry_cap) bytes (GF_ERR_CAPACITY when smaller).
 * Output: exactly that of gf_scan_pairs_device on the same pairs — one gf_pair_hit per matched read in push order
 * (pair, then merged | R1, R2) with the same source, flags, merge_diff, read_len and seq_offset, the matched reads'
 * bases and qualities in d_hit_bases / d_hit_quals, and d_totals (int64[8]): [0] hits, [1] bytes of their reads,
 * [2] pairs that merged, [3] reads searched again reversed, [4] overflow bits — 1: more retries than retry_cap (the
 * retry pass was emptied: run again with retry_cap = 3 n), 2: more hits or bytes than the output capacities ([0], [1]
 * say how many; the records that fit are the first of the full list) — [5..7] 0. */
int gf_mc_pairs_scan_device(const gf_index* idx, const void* d_prepared, const void* d_l_bases, const void* d_l_quals,
                            const void* d_l_offsets, int64_t l_bytes, const void* d_r_bases, const void* d_r_quals,
                            const void* d_r_offsets, int64_t r_bytes, int64_t n, int32_t max_read_len,
                            const void* d_gene_reversed, int32_t n_genes, int64_t pair_id_base, int64_t retry_cap,
                            void* d_workspace, int64_t workspace_bytes, void* d_hits, int64_t hits_cap, void* d_hit_bases,
                            void* d_hit_quals, int64_t hit_bytes_cap, void* d_totals, void* stream);

/* The message of the calling thread's last failed gf_mc_* call. */
const char* gf_mc_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* GF_MULTI_CSV_H */
