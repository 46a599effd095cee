/* gf_inflate — BGZF-compressed text inflated on the device: C ABI of libgfinflate.so.
 *
 * Sequencer output and every file written by bgzip is BGZF: a series of gzip members of at most 64 KiB of text each,
 * each with its compressed size in a `BC` extra subfield and its CRC-32 and text length (ISIZE) in its trailer.  The
 * members share no window, so a chunk of them is a data-parallel job.  The host walks the members' headers
 * (gf_if_walk_blocks: no GPU, no inflate) and copies the compressed bytes to the device as they are; there
 * gf_if_inflate_device decodes them, one wavefront a member, and checks each member's CRC-32.
 *
 * A member is BGZF when ID1 ID2 CM = 1f 8b 08, FLG = 4, and a `BC` subfield of length 2 is among its extra subfields
 * (others may come before it).  Empty members, the 28-byte end-of-file marker among them, are ordinary members with
 * ISIZE 0.
 *
 * A table row is int64[GF_IF_ROW_INT64]: [0] payload offset in the compressed bytes, [1] payload length, [2] text
 * offset in the output, [3] text length (ISIZE), [4] CRC-32, [5] the member's offset in the file (for messages).
 *
 * No gf_index is taken: the device is that of the pointers.  The library is built next to libgfmatch.so and links
 * against it like its siblings, but calls nothing of it on the device.  Conventions are those of gfmatch.h: plain
 * pointers and sizes, caller owns every buffer, GF_OK or a negative GF_ERR_* code, with a message for the calling thread
 * in gf_if_last_error().
 */
#ifndef GF_INFLATE_H
#define GF_INFLATE_H

#include "gfmatch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GF_IF_ROW_INT64 6

/* Why gf_if_walk_blocks stopped (result[3]). */
#define GF_IF_WALK_END 0      /* every byte of the range belongs to a whole member */
#define GF_IF_WALK_INSIDE 1   /* the range ends inside a member: its header, payload or trailer */
#define GF_IF_WALK_BUDGET 2   /* the next member's text would exceed text_budget */
#define GF_IF_WALK_CAPACITY 3 /* the table is full */
#define GF_IF_WALK_NOT_BGZF 4 /* what starts at result[4] is no BGZF member */

/* A member's status in d_status: 0 is a good member, the text inflated and its CRC-32 right.
 *    1 reserved block type       2 stored block: LEN != ~NLEN         3 HLIT > 286 or HDIST > 30
 *    4 over-subscribed code      5 incomplete code                    6 repeat code 16 with nothing before it
 *    7 code lengths past HLIT + HDIST                                 8 no end-of-block code
 *    9 literal/length symbol 286 or 287                              10 distance symbol 30 or 31
 *   11 distance beyond the member's own text                         12 more text than ISIZE
 *   13 less text than ISIZE     14 payload ends inside the stream    15 CRC-32 mismatch
 *   16 the table row points outside the compressed bytes or the output, or is longer than a BGZF member can be
 *   17 bits that are no code    18 payload bytes behind the final block */
#define GF_IF_STATUS_CRC 15
#define GF_IF_STATUS_BAD_ROW 16

/* Host code, no GPU: walks the BGZF members of comp[0, comp_bytes) by their headers and writes one table row per member
 * (table: int64[max_members][GF_IF_ROW_INT64]); payload offsets count from comp, text offsets from 0, the file offset
 * is file_offset + the member's offset in comp.  It stops before the member that would bring the text beyond
 * text_budget, or the rows beyond max_members.
 *   result (int64[5]): [0] members written, [1] compressed bytes they take (they are comp's first), [2] bytes of text
 *   they hold, [3] why the walk stopped (GF_IF_WALK_*), [4] the offset in comp where it stopped.
 * Bytes that are no BGZF member are reported (GF_IF_WALK_NOT_BGZF), they are no error: GF_ERR_ARG is for null pointers
 * and negative sizes only. */
int gf_if_walk_blocks(const void* comp, int64_t comp_bytes, int64_t file_offset, int64_t text_budget, int64_t max_members,
                      int64_t* table, int64_t* result);

/* Device bytes gf_if_inflate_device needs as d_workspace (the kernels keep a member's text in LDS: currently none, and
 * d_workspace may then be NULL). */
int64_t gf_if_workspace_bytes(int64_t n_members);

/* The members of d_table inflated, one asynchronous call queued on `stream` (a hipStream_t, NULL = default stream): no
 * host synchronisation, no allocation and no copy between host and device.  Every pointer is device memory on the device
 * of d_table (GF_ERR_NO_DEVICE when it is not device memory).
 *   d_comp: uint8[comp_bytes], the compressed bytes.  d_table: int64[n_members][GF_IF_ROW_INT64].
 *   d_out: uint8[out_cap]; a good member's text is written to its row's range, nothing else of d_out is: a member that
 *   fails writes nothing, and a row that points outside comp_bytes or out_cap is status 16 for that member, no fault.
 *   d_status: int32[n_members].
 *   d_totals: int64[4]: [0] members inflated, [1] the first failed member or -1, [2] its status, [3] bytes of text
 *   written. */
int gf_if_inflate_device(const void* d_comp, int64_t comp_bytes, const void* d_table, int64_t n_members, void* d_out,
                         int64_t out_cap, void* d_status, void* d_totals, void* d_workspace, int64_t workspace_bytes,
                         void* stream);

/* hipMemcpyAsync host -> device on `stream`, on the device of d_dst: gf_copy_from_host_device of gfmatch.h without an
 * index.  Asynchronous when h_src is pinned (gf_host_alloc). */
int gf_if_copy_from_host_device(const void* h_src, void* d_dst, int64_t nbytes, void* stream);

/* The message of the calling thread's last failed gf_if_* call. */
const char* gf_if_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* GF_INFLATE_H */
