/* gf_report — the report tail in bulk: C ABI of libgfreport.so.
 *
 * Every scan ends in the same tail: the three filters of FusionMapper::filter_matches, the first-fit clustering of
 * cluster_matches and the break refinement of FusionResult::adjust_fusion_break.  This library takes the matches of a
 * run as arrays — the reads' bases back to back, int64 offsets[n + 1] (read i is bases[offsets[i], offsets[i + 1])),
 * gf_readmatch[n] — and does the per-match work on the device, all matches in one call, and the sequential part of
 * the clustering on the host in time linear in the matches.
 *
 * No gf_index is taken: the device is that of the pointers.  The library is built next to libgfmatch.so and links
 * against it like its siblings, but calls nothing of it on the device.  Conventions are those of gfmatch.h: plain
 * pointers and sizes, caller owns every buffer, GF_OK or a negative GF_ERR_* code, with a message for the calling thread
 * in gf_rp_last_error().  The device calls are asynchronous: queued on `stream` (a hipStream_t, NULL = default stream),
 * no host synchronisation, no allocation, no copy between host and device, no workspace.
 */
#ifndef GF_REPORT_H
#define GF_REPORT_H

#include "gfmatch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A match's status in gf_rp_adjust_device's output. */
#define GF_RP_STATUS_OK 0
#define GF_RP_STATUS_OUT_OF_DOMAIN 1 /* read_break < 3 or read_break > len - 5: a shift of -3 .. 3 would leave a side of
                                        the read empty, where the reference's skip / take have quirks of their own; the
                                        match is not computed (the filter never lets such a match through) */
#define GF_RP_STATUS_BAD_ROW 2       /* offsets, cluster or reference offsets outside their arrays, or a read longer
                                        than GF_MAX_READ_LEN: nothing was read through them */

/* Negative filter reasons. */
#define GF_RP_REASON_BAD_BREAK (-1) /* read_break + 1 outside [0, len] (gf_readmatch_filter: GF_ERR_ARG) */
#define GF_RP_REASON_BAD_READ (-2)  /* offsets outside d_bases, or a read longer than GF_MAX_READ_LEN */

/* gf_readmatch_filter for n matches: d_reason (int32[n]) gets 0 = kept, 1 = low complexity (a side of the break
 * shorter than 20 bases or with fewer than 7 unequal neighbouring symbols), 2 = left_distance + right_distance >= 5,
 * 3 = same contig and |left_position - right_position| < deletion_threshold, tested in that order; or a negative
 * GF_RP_REASON_*, and then nothing was read out of bounds.
 *   d_bases: uint8[bases_bytes].  d_offsets: int64[n + 1].  d_matches: gf_readmatch[n]. */
int gf_rp_filter_device(const void* d_bases, int64_t bases_bytes, const void* d_offsets, const void* d_matches, int64_t n,
                        int32_t deletion_threshold, void* d_reason, void* stream);

/* FusionResult::adjust_fusion_break for n matches of n_clusters clusters.
 *   d_cluster: int32[n], the cluster of each match.
 *   d_refs: uint8[refs_bytes], the clusters' references back to back; d_ref_offsets: int64[2 * n_clusters + 1]: cluster
 *   c's left reference (m_left_ref) is d_refs[d_ref_offsets[2 c], d_ref_offsets[2 c + 1]), its right reference
 *   (m_right_ref) the range after it.  Either may be empty.
 *   d_out: int32[n][4] = {shift, left_distance, right_distance, status}: the first shift in the order -3 .. 3 whose
 *   20-base total is strictly smallest, and the whole-overlap distances at that shift; the first three are 0 unless
 *   status is GF_RP_STATUS_OK. */
int gf_rp_adjust_device(const void* d_bases, int64_t bases_bytes, const void* d_offsets, const void* d_matches,
                        const void* d_cluster, int64_t n, const void* d_refs, int64_t refs_bytes,
                        const void* d_ref_offsets, int64_t n_clusters, void* d_out, void* stream);

/* Host code, no GPU: the first-fit clustering of cluster_matches for n_groups lists of matches, without scanning the
 * clusters.  Group g is the matches [group_off[g], group_off[g + 1]) in their sorted order, group_off[0] = 0; lp / rp
 * (int32 each) are their left and right positions.  founder_out (int64[group_off[n_groups]]) gets, per match, the
 * index of the match that founded the cluster it joins: the first cluster of its group, in the order the clusters were
 * made, that holds a match within 3 of it on both sides.  A match that founds a cluster names itself. */
int gf_rp_first_fit(const int32_t* lp, const int32_t* rp, const int64_t* group_off, int64_t n_groups,
                    int64_t* founder_out);

/* The message of the calling thread's last failed gf_rp_* call. */
const char* gf_rp_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* GF_REPORT_H */
