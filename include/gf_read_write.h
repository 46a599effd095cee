/* gf_read_write — the records that pass the preparation steps formatted as FASTQ text on the device: C ABI of
 * libgfwrite.so.
 *
 * The adapter trimming, the read filter, the duplicate removal and the UMI cut (gf_adapter_trim.h, gf_read_filter.h,
 * gf_dedup.h, gf_umi.h) leave the cleaned records in HBM for the length of one chunk, and only the scan sees them.
 * Other tools of a pipeline — an aligner, a variant caller — want the same records as files.  This call formats them
 * where they are: the chunk's text (for the name lines), its newline index and the records are all on the device, and
 * what leaves is FASTQ text, one device-to-host copy per side away from a file.  A feature outside the reference, and
 * nothing calls it unless asked to.
 *
 * The predicate.  Side s of record i (pairs: R1 and R2; single-end input: one side).  L(s, i) is the record's length
 * after all preparation steps: off[i + 1] - off[i] of that side's final offsets, 0 when that is negative.
 *
 *   When a record is written.  Record i is written when L(s, i) > 0 and, for pairs, its mate's is too.  Otherwise
 *     neither mate is written.
 *   Order.  Written records keep file order, and both sides write the same set of i: R1 and R2 stay in step.
 *   The four lines.  A written record is these bytes, back to back: its name line, with the tag if there is one, '\n';
 *     its bases as the last step left them, '\n'; "+\n"; its qualities, '\n'.
 *   The name line is what gf_hit_names.h defines: line 4 i of that side's text, from the byte after newline 4 i - 1
 *     (byte 0 for i = 0) up to, not including, newline 4 i, or to the end of the text when it has only 4 i newlines.
 *     The bytes are verbatim; a '\r' stays wherever the cut leaves it.  A record whose line the text does not have
 *     (4 i > newlines) has an empty name line.
 *   The tag.  With settings.umi_source one of GF_UM_READ1, GF_UM_READ2, GF_UM_PER_READ (gf_umi.h) and umi_length 1 ..
 *     GF_UM_MAX_LEN a tag is inserted at the end of the name line's first token: before the first space or tab, or at
 *     the line's end.  The tag is ':' + UMI.  For READ1 or READ2 the UMI is the first umi_length bases of the taking
 *     mate as they stood before the cut (the pre-cut batches; a pre-cut record shorter than that gives what it has);
 *     for PER_READ on pairs it is umi1 + '_' + umi2; with single-end input PER_READ is READ1 and READ2 is refused.
 *     Both mates of a pair get the same tag, and the case of the bytes is kept.  umi_source GF_UM_NAME (0): no tag, and
 *     umi_length must be 0 — the name source's UMI is in the name already.
 *   Output size.  A written record is name + tag + 2 L + 5 bytes and never longer than its input record + 1 + the tag
 *     (the + 1: a text without a final newline), so GF_RW_CAPACITY(text_bytes, n) is a capacity the host knows without
 *     a read-back; below it the call returns GF_ERR_CAPACITY, and there is no overflow retry.  Should final records
 *     be handed in that are longer than the text's, the records that do not fit are left out of the text (their
 *     offsets and the totals still count them: a side's bytes above out_cap say so) and nothing outside the
 *     buffer is written.
 *
 * d_out_off (int64[n + 1], from 0): record i's bytes are d_out_text[off[i] .. off[i + 1]), none for a record that is
 * not written; off[n] is the side's output size.
 *
 * d_totals (int64[GF_RW_TOTALS]) is ADDED into, never zeroed: [0] records written, in the scan's own units (pairs or
 * reads), [1] bases written, both mates', [2] output bytes of side 0, [3] of side 1, [4] records not written.
 *
 * Known answer: the record "@r1 x", "ACGT", "+", "FFFF" cut to "GT" / "FF" behind the UMI "AC" of READ1 is written as
 * "@r1:AC x\nGT\n+\nFF\n".
 *
 * A library of its own on top of libgfmatch.so (it uses gf_index_info_get of gfmatch.h to find the index's device).
 * Conventions are those of gf_umi.h: plain pointers and sizes, caller owns every buffer, GF_OK or a negative GF_ERR_*
 * code, with a message for the calling thread in gf_rw_last_error().  The device call is one asynchronous call queued
 * on `stream` (a hipStream_t, NULL = default stream): no host synchronisation, no allocation by this library and no
 * copy between host and device.  There is no CPU fallback: host memory is refused (GF_ERR_NO_DEVICE).  As in gfmatch.h
 * the kernel loads whole aligned 16-byte chunks around a name line and a record's bases and qualities: up to 15 bytes
 * before the first and past the last byte are READ (never written, never interpreted).  No byte outside a record's own
 * output span is written.  Offsets are 64-bit throughout.  Deterministic.
 */
#ifndef GF_READ_WRITE_H
#define GF_READ_WRITE_H

#include "gf_umi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GF_RW_TAG_MAX (1 + 32 + 1 + 32)
#define GF_RW_TOTALS 5
/* the output capacity of a side with a text of text_bytes bytes and n records */
#define GF_RW_CAPACITY(text_bytes, n) ((int64_t)(text_bytes) + 1 + (int64_t)(n) * GF_RW_TAG_MAX)

#define GF_RW_WIDE 0  /* the output assembled in aligned 16-byte pieces, one store a piece */
#define GF_RW_BYTES 1 /* the same bytes, one per lane and store: kept to measure the other against */

typedef struct gf_rw_settings {
  int32_t umi_source; /* GF_UM_NAME (0): no tag; GF_UM_READ1, GF_UM_READ2, GF_UM_PER_READ: the tag */
  int32_t umi_length; /* 0 without a tag, else 1 .. GF_UM_MAX_LEN */
  int32_t gather;     /* GF_RW_WIDE or GF_RW_BYTES: the same output either way */
} gf_rw_settings;

/* One side of the call.  The text the records were cut from and its newline index (as gf_fastq_index_device wrote
 * it); the final batch as the last preparation step left it (bases, qualities at the bases' offsets, offsets
 * int64[n + 1] that need not start at 0); the pre-cut batch's bases and offsets, as gf_um_cut_device took them, both
 * sides' with a tag and NULL without; and the output. */
typedef struct gf_rw_side {
  const void* d_text;
  int64_t text_bytes;
  const void* d_nl_pos;
  int64_t newlines;
  const void* d_bases;
  const void* d_quals;
  const void* d_off;
  const void* d_pre_bases;
  const void* d_pre_off;
  void* d_out_text; /* uint8[out_cap] */
  int64_t out_cap;  /* >= GF_RW_CAPACITY(text_bytes, n) */
  void* d_out_off;  /* int64[n + 1] */
} gf_rw_side;

/* Device bytes gf_rw_format_device needs as d_workspace for n records.  Non-decreasing in n. */
int64_t gf_rw_workspace_bytes(int64_t n);

/* The n records of `left` — with `right` (NULL for single-end input) the n pairs of both — formatted.  d_workspace:
 * gf_rw_workspace_bytes(n) bytes (GF_ERR_CAPACITY when smaller). */
int gf_rw_format_device(const gf_index* idx, const gf_rw_settings* settings, const gf_rw_side* left,
                        const gf_rw_side* right, int64_t n, void* d_workspace, int64_t workspace_bytes, void* d_totals,
                        void* stream);

/* The message of the calling thread's last failed gf_rw_* call. */
const char* gf_rw_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* GF_READ_WRITE_H */
