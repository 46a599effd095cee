/* gf_ref_cut — the gene slices of a reference FASTA, cut out on the device chunk by chunk: C ABI of libgfrefcut.so.
 *
 * gf_index_build takes the gene slices already cut; FastaReader::read_all (fasta_reader.rs:121-201) and
 * Indexer::make_index (indexer.rs:137-158) get them by reading the whole FASTA into a map of contigs first.  Here a
 * chunk of the FASTA's text lies in HBM; gf_rc_index_device finds its records and counts its sequence bytes,
 * gf_rc_gather_device writes the bytes of the wanted ranges, upper-cased.  The host keeps the record names, decides
 * which ranges it wants (genefuserust_amd/ref_cut.py) and never holds the file.
 *
 * The rules are those of the reader: every '>' starts a record, even one inside a header line; a record's name runs
 * from its '>' to the first '\n' or ' ', which is consumed; every byte from there to the next '>' is a sequence
 * candidate, and is kept when it is an ASCII letter, '-' or '*'.
 *
 * Records of a chunk are numbered by ordinal: 0 is the record the chunk starts in (the one carried in from the previous
 * chunk; at the start of a file: the bytes that belong to nothing), k >= 1 the record started by the chunk's k-th '>'.
 * A byte's kept rank is the number of letters, '-' and '*' before it in the chunk, name bytes included: one plain
 * scan.  Its position in its contig is its rank minus the rank at its record's sequence start; a name byte comes out
 * negative and is no sequence.
 *
 * No gf_index exists when a reference is cut, so nothing here takes one: the device is that of the text pointer.  The
 * library is built next to libgfmatch.so and links against it like its siblings, but calls nothing of it on the
 * device.  Conventions are those of gfmatch.h: plain pointers and sizes, caller owns every buffer, GF_OK or a negative
 * GF_ERR_* code, with a message for the calling thread in gf_rc_last_error().
 */
#ifndef GF_REF_CUT_H
#define GF_REF_CUT_H

#include "gfmatch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of text per tile of the kernels: counts are kept per tile, a block takes a tile. */
int64_t gf_rc_tile_bytes(void);
/* Tiles a text of text_bytes can touch: the tiles lie on the 16-byte grid of addresses, so a text that starts off the
 * grid can touch one more than text_bytes / gf_rc_tile_bytes() rounded up. */
int64_t gf_rc_tiles(int64_t text_bytes);
/* Device bytes gf_rc_index_device needs as d_workspace.  Non-decreasing in text_bytes. */
int64_t gf_rc_workspace_bytes(int64_t text_bytes);

/* One interval of gf_rc_gather_device: the kept bytes at contig positions [start, end) of record `record` (its ordinal
 * in the chunk) go to d_out[out_offset .. out_offset + end - start). */
typedef struct gf_rc_interval {
  int64_t record, start, end, out_offset;
} gf_rc_interval;

/* The records of a chunk of FASTA text, one asynchronous call queued on `stream` (a hipStream_t, NULL = default
 * stream): no host synchronisation, no allocation and no copy between host and device.  Every pointer is device memory
 * on the device of d_text (GF_ERR_NO_DEVICE when d_text is not device memory).
 *   d_text: uint8[text_bytes], any alignment.
 *   d_workspace: gf_rc_workspace_bytes(text_bytes) bytes (GF_ERR_CAPACITY when smaller).
 * Output, for the records k = 1 .. min(records, cap_records) at index k - 1, '>' positions ascending:
 *   d_gt_pos   (int64[cap_records]): where the record's '>' is.
 *   d_gt_rank  (int64[cap_records]): the kept rank at its '>' — where the record before it ends.
 *   d_name_end (int64[cap_records]): where its name's delimiter is (the first '\n' or ' ' before the next '>' and the
 *              end of the text), -1 when it is not in this chunk.
 *   d_seq_rank (int64[cap_records]): the kept rank at its sequence start, the byte after the delimiter; without a
 *              delimiter the rank at the record's end, which makes the sequence empty.
 *   d_name_off (int64[cap_records + 1]) / d_names (uint8[names_cap]): the names back to back, name k - 1 at
 *              d_name_off[k - 1] .. d_name_off[k]; a name is written only when all of it fits names_cap, the offsets
 *              are always the true ones.
 *   d_tile_kept (int64[gf_rc_tiles(text_bytes) + 1]): the kept rank at the start of every tile, and the total.
 *   d_totals (int64[8]): [0] records started in the chunk, [1] kept bytes, [2] overflow bits — 1: more records than
 *              cap_records, 2: the names take more than names_cap bytes — [3] where an unfinished header begins (the
 *              '>' of the last record, when its name's delimiter is not in the chunk; -1 when there is none), [4] bytes
 *              of all names.  With overflow bit 1 the per-record outputs hold the first cap_records records and [3],
 *              [4] are not to be used: run again with room for [0] records. */
int gf_rc_index_device(const void* d_text, int64_t text_bytes, int64_t cap_records, void* d_workspace,
                       int64_t workspace_bytes, void* d_gt_pos, void* d_gt_rank, void* d_name_end, void* d_seq_rank,
                       void* d_name_off, void* d_names, int64_t names_cap, void* d_tile_kept, void* d_totals,
                       void* stream);

/* The kept bytes of the wanted ranges, upper-cased; asynchronous like gf_rc_index_device, whose outputs for the same
 * text it takes: d_gt_pos, d_seq_rank, d_tile_kept.  n_records: how many records of the chunk to know of (at most what
 * the index call wrote); text_bytes may be smaller than it was for the index call (a text cut off in front of an
 * unfinished header).  carried_kept: what record 0 had already kept before this chunk.
 *   d_intervals: gf_rc_interval[n_intervals], disjoint, sorted by record and start.
 * Every kept byte whose contig position p falls in an interval is written to d_out[out_offset + p - start] when that
 * index is below out_cap (uint8[out_cap]); nothing else of d_out is written. */
int gf_rc_gather_device(const void* d_text, int64_t text_bytes, const void* d_gt_pos, const void* d_seq_rank,
                        int64_t n_records, const void* d_tile_kept, int64_t carried_kept, const void* d_intervals,
                        int64_t n_intervals, void* d_out, int64_t out_cap, void* stream);

/* hipMemcpyAsync host -> device on `stream`, on the device of d_dst: gf_copy_from_host_device of gfmatch.h without an
 * index.  Asynchronous when h_src is pinned (gf_host_alloc). */
int gf_rc_copy_from_host_device(const void* h_src, void* d_dst, int64_t nbytes, void* stream);

/* The message of the calling thread's last failed gf_rc_* call. */
const char* gf_rc_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* GF_REF_CUT_H */
