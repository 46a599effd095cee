/* gf_scan_pack — the outputs of K scans and their names packed into one dense block on the device: C ABI of
 * libgfpack.so.
 *
 * A scan (gf_scan_pairs_device, gf_se_scan_device, gf_mc_pairs_scan_device) leaves its records, the matched reads and
 * its totals in four buffers, and gf_hn_names_device leaves the names in three more; the counts are on the device.  A
 * host that scans one chunk of reads against K indexes would fetch 7 K buffers with K round trips.  This call gathers
 * what the K scans really produced — nothing beyond their counts — into one block with a header, so that the host
 * fetches the header and then exactly the bytes that are there: two copies, whatever K is.
 *
 * A library of its own next to libgfmatch.so; it takes no gf_index and finds its device from d_block.  Conventions are
 * those of gfmatch.h: plain pointers and sizes, caller owns every buffer, GF_OK or a negative GF_ERR_* code, with a
 * message for the calling thread in gf_pk_last_error().
 */
#ifndef GF_SCAN_PACK_H
#define GF_SCAN_PACK_H

#include "gfmatch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GF_PK_MAX_SCANS 1024 /* K of one call */

/* Overflow bits of a scan's header ([7], low byte). */
#define GF_PK_OVER_RETRY 1 /* the scan's own bit 1: more retries than retry_cap */
#define GF_PK_OVER_HITS 2  /* the scan's own bit 2: more hits / bytes than its output capacities */
#define GF_PK_OVER_NAMES 4 /* the names did not fit names_cap */
#define GF_PK_BAD_SCAN 8   /* the descriptor does not hold together (see gf_pk_pack_device) */

/* One scan and its names, as they lie in HBM.  Every pointer is device memory. */
typedef struct gf_pk_scan {
  const void* d_hits;        /* gf_pair_hit[hits_cap] */
  const void* d_bases;       /* uint8[bytes_cap]: the matched reads, at seq_offset */
  const void* d_quals;       /* uint8[bytes_cap] */
  const void* d_totals;      /* int64[8], the layout of gf_scan_pairs_device */
  const void* d_names;       /* uint8[names_cap], as gf_hn_names_device wrote it */
  const void* d_name_off;    /* int64[hits_cap + 1] */
  const void* d_name_totals; /* int64[4], the layout of gf_hn_names_device */
  int64_t hits_cap, bytes_cap, names_cap;
} gf_pk_scan;

/* Bytes of a block that holds k scans with `records` records, `read_bytes` bytes of matched reads (the bases; the
 * qualities take as many again) and `name_bytes` bytes of names in all.  Non-decreasing in every argument; 0 for a
 * negative one.  With the true sums of scans that all fit it is exactly what gf_pk_pack_device needs (a scan packed
 * as empty takes less). */
int64_t gf_pk_block_bytes(int64_t k, int64_t records, int64_t read_bytes, int64_t name_bytes);

/* Device bytes gf_pk_pack_device needs as d_workspace for k scans.  Non-decreasing in k; 0 for a negative one. */
int64_t gf_pk_workspace_bytes(int64_t k);

/* The block of k scans, one asynchronous call queued on `stream` (a hipStream_t, NULL = default stream): no host
 * synchronisation, no allocation by this library and no copy between host and device.
 *   d_scans: gf_pk_scan[k] in device memory, 1 <= k <= GF_PK_MAX_SCANS.
 *   d_workspace: gf_pk_workspace_bytes(k) bytes (GF_ERR_CAPACITY when smaller).
 *   d_block (16-byte aligned) / block_bytes: the block; it has to hold the headers, 64 (k + 1) bytes
 *     (GF_ERR_CAPACITY when smaller).
 * GF_ERR_ARG, before a device is touched: k outside its range, a null d_scans / d_workspace / d_block, a negative
 * size, a d_block off the 16-byte grid.
 *
 * The block — every section starts on a 16-byte boundary, and the bytes between a section's end and the next
 * boundary are written as zero, so that two blocks can be compared whole:
 *   int64[8]     [0] bytes of the body, [1] k, [2] overflow: 1 when 64 (k + 1) + [0] is more than block_bytes — then the
 *                headers are valid, and nothing else is written; pack again with that many bytes.  [3] .. [7] zero.
 *   int64[k][8]  per scan: [0] records, [1] read bytes and [2] name bytes that were packed, [3] the scan's merged_pairs
 *                (totals[2]), [4] its retried_reads (totals[3]), [5] its true hit count (totals[0]), [6] records without
 *                a name line (name totals[3]), [7] the GF_PK_* bits, and above them ([7] >> 8) the bytes the names
 *                take (name totals[1]).
 *   the body     five sections, each with the scans 0 .. k - 1 back to back: the gf_pair_hit records; the bases; the
 *                qualities; the name offsets (int64[records + 1] per scan, counted from the scan's own first name);
 *                the names.  A record's seq_offset stays relative to its own scan's part of the bases section.
 * The counts are read on the device and clamped to the capacities: records = min(totals[0], hits_cap), and so on; no
 * row, byte or offset beyond a scan's counts reaches the block.  A scan with any GF_PK_* bit is packed as empty —
 * nothing in any section, not even its one name offset — and its header says which scan to run again (GF_PK_OVER_RETRY,
 * GF_PK_OVER_HITS: with more room; GF_PK_OVER_NAMES: the names with [7] >> 8 bytes).  GF_PK_BAD_SCAN: a count beyond
 * its capacity without the scan's own bit, a negative capacity, a null pointer where the count is not zero, names of
 * another number of records, or a first name offset outside the names. */
int gf_pk_pack_device(const void* d_scans, int64_t k, void* d_workspace, int64_t workspace_bytes, void* d_block,
                      int64_t block_bytes, void* stream);

/* The message of the calling thread's last failed gf_pk_* call. */
const char* gf_pk_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* GF_SCAN_PACK_H */
