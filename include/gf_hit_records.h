/* gf_hit_records — the original FASTQ records of the reads a scan matched, gathered on the device: the second gather
 * of libgfnames.so, next to gf_hn_names_device (gf_hit_names.h).
 *
 * The HTML report shows, under every supporting read, the FASTQ records it came from (ReadMatch::m_original_reads:
 * both mates of a pair whichever read matched, pescanner.rs:456-511; the one read of single-end input,
 * sescanner.rs:191-197).  A streamed scan drops a chunk's text as soon as the chunk is scanned, so the records of the
 * hit records are copied out of the text while it is still in HBM.
 *
 * Conventions are those of gf_hit_names.h, errors are reported through gf_hn_last_error().
 */
#ifndef GF_HIT_RECORDS_H
#define GF_HIT_RECORDS_H

#include "gf_hit_names.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device bytes gf_hn_records_device needs as d_workspace for hits_cap records (of either layout).  Non-decreasing in
 * hits_cap. */
int64_t gf_hn_records_workspace_bytes(int64_t hits_cap);

/* The FASTQ records of the hit records, one asynchronous call queued on `stream`: no host synchronisation, no
 * allocation by this library and no copy between host and device, so that the call can be captured into a graph.
 * d_hits / d_totals / hits_cap / pair_id_base and the two texts with their newline indexes are what gf_hn_names_device
 * takes; d_r_text NULL (with 0 sizes) is single-end input.
 *   S = 2 with d_r_text, else 1.  Hit record k, FASTQ record i = pair_id - pair_id_base, side s (0: R1, 1: R2): the
 *   span from the byte after newline 4i - 1 (byte 0 for i = 0) up to, not including, newline 4i + 3 (the end of the
 *   text when it has fewer newlines): the record's four lines joined by their own '\n', without the last one.  Both
 *   sides are gathered for every record, whatever its `source`.  Start and end are clamped to the text.
 *   d_workspace: gf_hn_records_workspace_bytes(hits_cap) bytes (GF_ERR_CAPACITY when smaller).
 * Output: the spans back to back in d_records (uint8[records_cap]), span (k, s) at d_record_off[S k + s] ..
 * d_record_off[S k + s + 1] (int64[S hits_cap + 1]; entries beyond the number of spans + 1 are not written).  A span
 * is written only when all of it fits records_cap; the offsets are always the true ones.  A span whose i is not on
 * its text (i < 0 or i > newlines / 4) is empty and is counted.
 * d_record_totals (int64[4]): [0] spans (S times the records), [1] bytes of all spans, [2] overflow bits — 1:
 * records_cap is smaller than [1] (run again with that many bytes) — [3] spans without a record. */
int gf_hn_records_device(const gf_index* idx, const void* d_hits, const void* d_totals, int64_t hits_cap,
                         int64_t pair_id_base, const void* d_l_text, int64_t l_text_bytes, const void* d_l_nl_pos,
                         int64_t l_newlines, const void* d_r_text, int64_t r_text_bytes, const void* d_r_nl_pos,
                         int64_t r_newlines, void* d_workspace, int64_t workspace_bytes, void* d_records,
                         int64_t records_cap, void* d_record_off, void* d_record_totals, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GF_HIT_RECORDS_H */
