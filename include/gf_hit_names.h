/* gf_hit_names — the names of the reads a scan matched, gathered on the device: C ABI of libgfnames.so.
 *
 * A scan (gf_scan_pairs_device, gf_se_scan_device, gf_mc_pairs_scan_device) leaves gf_pair_hit records with the
 * matched reads' bases and qualities; the one thing a ReadMatch still needs from the FASTQ text is the read's name
 * (SequenceRead.m_name, read.rs:17-23).  This call copies the name lines of the hit records out of the text while it
 * is still in HBM, so that a chunk of a streamed FASTQ can be dropped as soon as it is scanned.
 *
 * A library of its own on top of libgfmatch.so (it uses gf_index_info_get of gfmatch.h to find the index's device).
 * Conventions are those of gfmatch.h: plain pointers and sizes, caller owns every buffer, GF_OK or a negative GF_ERR_*
 * code, with a message for the calling thread in gf_hn_last_error().
 */
#ifndef GF_HIT_NAMES_H
#define GF_HIT_NAMES_H

#include "gfmatch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device bytes gf_hn_names_device needs as d_workspace for hits_cap records.  Non-decreasing in hits_cap. */
int64_t gf_hn_workspace_bytes(int64_t hits_cap);

/* The name lines of the hit records, one asynchronous call queued on `stream` (a hipStream_t, NULL = default
 * stream): no host synchronisation, no allocation by this library and no copy between host and device, so that the
 * call can be captured into a graph.  Every pointer is device memory on the index's device.
 *   d_hits / d_totals: the gf_pair_hit records and the totals a scan wrote; the number of records is
 *     min(d_totals[0], hits_cap) and is read on the device.
 *   pair_id_base: what the scan was given; record k names FASTQ record i = pair_id - pair_id_base.
 *   d_l_text (uint8[l_text_bytes]) and d_l_nl_pos (int64[l_newlines], as gf_fastq_index_device wrote it): the FASTQ
 *     text of R1 and the byte offsets of its newlines; d_r_text / d_r_nl_pos / r_text_bytes / r_newlines the same for
 *     R2, all NULL / 0 for single-end input.  A record with source == 2 takes its name from R2, any other from R1.
 *   d_workspace: gf_hn_workspace_bytes(hits_cap) bytes (GF_ERR_CAPACITY when smaller).
 * Output, in record order: the name line of record i — from the byte after newline 4i - 1 (byte 0 for i = 0) up to,
 * not including, newline 4i (the end of the text when the text has only 4i newlines) — back to back in d_names
 * (uint8[names_cap]), name k at d_name_off[k] .. d_name_off[k + 1] (int64[hits_cap + 1]; entries beyond the number of
 * records + 1 are not written).  A name is written only when all of it fits names_cap; the offsets are always the true
 * ones.  A record whose i is no line of its text (or whose text is NULL) gets an empty name and is counted.
 * d_name_totals (int64[4]): [0] names, [1] bytes of all names, [2] overflow bits — 1: names_cap is smaller than [1]
 * (run again with that many bytes) — [3] records without a name line. */
int gf_hn_names_device(const gf_index* idx, const void* d_hits, const void* d_totals, int64_t hits_cap,
                       int64_t pair_id_base, const void* d_l_text, int64_t l_text_bytes, const void* d_l_nl_pos,
                       int64_t l_newlines, const void* d_r_text, int64_t r_text_bytes, const void* d_r_nl_pos,
                       int64_t r_newlines, void* d_workspace, int64_t workspace_bytes, void* d_names,
                       int64_t names_cap, void* d_name_off, void* d_name_totals, void* stream);

/* The message of the calling thread's last failed gf_hn_* call. */
const char* gf_hn_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* GF_HIT_NAMES_H */
