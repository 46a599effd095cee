/* gf_umi — unique molecular identifiers cut on the device and keyed into the duplicate removal: C ABI of libgfumi.so.
 *
 * Deep cell-free-DNA panels carry unique molecular identifiers (UMIs): a few random bases ligated to a molecule before
 * the PCR, read as the first bases of R1, R2 or both (often followed by a spacer), or written by the sequencer's
 * software behind the last ':' of the read's name.  cfDNA is cut at preferred positions, so two distinct molecules with
 * the same bases are common at panel depth, and only the UMI tells a PCR copy from a second molecule.  These calls take
 * the inline UMIs off records that already sit in HBM, give every record a 64-bit code of its UMI, and mix that code
 * into the keys of the duplicate removal (gf_dedup.h).  A feature outside the reference, and nothing calls it unless
 * asked to.
 *
 * The predicate.  H, mix and fold are those of gf_dedup.h; arithmetic is mod 2^64.
 *
 * Inline sources (GF_UM_READ1, GF_UM_READ2, GF_UM_PER_READ), at any record length, also above GF_MAX_READ_LEN.  A side
 * takes a UMI when the source names it: READ1 the left side, READ2 the right side, PER_READ both; with single-end input
 * PER_READ is READ1 and READ2 is refused.  c = length + skip.
 *   a taking side whose record has L >= c: its UMI u is bytes [0, length) of the bases, and the record becomes bytes
 *     [c, L) of the bases and of the qualities, which may be none.
 *   a taking side with L < c, an empty record included: no UMI; the record becomes a record of length 0 and so does
 *     its mate, and the pair (or read) is counted once as too short for the UMI.
 *   a side that takes no UMI passes as it is, unless its mate emptied it.
 *   the code U of a record that stays: READ1 / READ2: U = H(u); PER_READ on pairs: U = mix(H(u1) + mix(H(u2) + 1)).
 *     A U of 0 becomes 1.  An emptied pair (or read) has U = 0.
 * Record count, order and indices stay.
 *
 * The name source (GF_UM_NAME) moves no byte of the records.  The name line of record i is what gf_hit_names.h
 * defines: line 4 i of the text, from the byte after newline 4 i - 1 (byte 0 for i = 0) up to, not including, newline
 * 4 i, or to the end of the text when it has only 4 i newlines; for pairs it is R1's line only.  One trailing '\r' is
 * stripped.  The first token ends at the first space or tab, or at the line's end.  The field is the token's bytes
 * behind its last ':'.  The field is a UMI when there is a ':' in the token, the field is 1 to GF_UM_MAX_FIELD (64)
 * bytes, and every byte is one of "ACGTNacgtn+_".  Then U = H(field) — fold makes "acgt" and "ACGT" equal — and a U of 0
 * becomes 1.  Otherwise U = 0 and the record is counted as without a UMI; so is a record whose line does not exist in
 * the text (4 i > newlines).
 *
 * The key.  With a code, the dedup key of a record with K != 0 and U != 0 is K' = mix(K + mix(U + 2)), and a K' of 0
 * becomes 1.  K == 0 stays 0.  With U == 0 the key stays K: a record without a UMI is deduplicated by its bases.
 *
 * Known answers: U("ACGTACGT") = U("acgtacgt") = 0x1d189c7f508326f9; U of the pair ("ACGT", "TTGA") =
 * 0x8a0ec19742ea7304; U of the name field "ACGT+TTGA" = 0xdecfd2a34e770449; K' of the bases "ACGT"
 * (K = 0xab0fcab10dd0c6f9) with these codes: 0xff1a16f0056acf7f, 0xf6e69183b4f4f21c, 0xc7033d0180ee6594.
 *
 * A library of its own on top of libgfmatch.so (it uses gf_index_info_get of gfmatch.h to find the index's device).
 * Conventions are those of gf_dedup.h: plain pointers and sizes, caller owns every buffer, GF_OK or a negative GF_ERR_*
 * code, with a message for the calling thread in gf_um_last_error().  Every device call is one asynchronous call
 * queued on `stream` (a hipStream_t, NULL = default stream): no host synchronisation, no allocation by this library
 * and no copy between host and device.  There is no CPU fallback: host memory is refused (GF_ERR_NO_DEVICE).  As in
 * gfmatch.h the kernels load whole aligned 16-byte chunks around a record's UMI and around a name line: up to 15 bytes
 * before its first and past its last byte are READ (never written, never interpreted).  Deterministic: every sum is an
 * integer.
 */
#ifndef GF_UMI_H
#define GF_UMI_H

#include "gfmatch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GF_UM_NAME 0
#define GF_UM_READ1 1
#define GF_UM_READ2 2
#define GF_UM_PER_READ 3
#define GF_UM_MAX_LEN 32
#define GF_UM_MAX_SKIP 32
#define GF_UM_MAX_FIELD 64
#define GF_UM_TOTALS 7

/* Inline sources need 1 <= length <= GF_UM_MAX_LEN and 0 <= skip <= GF_UM_MAX_SKIP; GF_UM_NAME needs length == 0 and
 * skip == 0.  Anything else is refused with GF_ERR_ARG. */
typedef struct gf_um_settings {
  int32_t source;
  int32_t length;
  int32_t skip;
} gf_um_settings;

/* d_totals (int64[GF_UM_TOTALS]) is ADDED into, never zeroed; in the scan's own units (pairs or reads): [0] records
 * seen, [1] records with a UMI (U != 0), [2] records without one (name source), [3] records whose UMI (for a pair:
 * either of the two) holds an 'N' or 'n', [4] bases cut off, both mates', for the records that stay, [5] records
 * emptied as too short for the UMI, [6] bases removed with those. */

/* Device bytes gf_um_cut_device needs as d_workspace for n records.  Non-decreasing in n. */
int64_t gf_um_workspace_bytes(int64_t n);

/* The inline sources: settings->source one of GF_UM_READ1, GF_UM_READ2, GF_UM_PER_READ (GF_ERR_ARG for GF_UM_NAME, and
 * for GF_UM_READ2 with single-end input).  Input as gf_pp_filter_device takes it (bases, qualities at the bases'
 * offsets, offsets int64[n + 1] that need not start at 0; the mates' three NULL for single-end input); output as it
 * writes it: the records that stay, cut, back to back in d_*_out_bases / d_*_out_quals (as many bytes as the records
 * had), record i at d_*_out_off[i] .. d_*_out_off[i + 1] (int64[n + 1], from 0).  d_codes (uint64[n]): U of every
 * record.  d_workspace: gf_um_workspace_bytes(n) bytes (GF_ERR_CAPACITY when smaller). */
int gf_um_cut_device(const gf_index* idx, const gf_um_settings* settings, const void* d_l_bases, const void* d_l_quals,
                     const void* d_l_off, const void* d_r_bases, const void* d_r_quals, const void* d_r_off, int64_t n,
                     void* d_workspace, int64_t workspace_bytes, void* d_l_out_bases, void* d_l_out_quals,
                     void* d_l_out_off, void* d_r_out_bases, void* d_r_out_quals, void* d_r_out_off, void* d_codes,
                     void* d_totals, void* stream);

/* The name source: U of the n records whose name lines are the lines 0, 4, .. 4 (n - 1) of d_text (uint8[text_bytes]);
 * d_nl_pos (int64[newlines], as gf_fastq_index_device wrote it): the byte offsets of its newlines.  d_codes
 * (uint64[n]). */
int gf_um_names_device(const gf_index* idx, const void* d_text, int64_t text_bytes, const void* d_nl_pos,
                       int64_t newlines, int64_t n, void* d_codes, void* d_totals, void* stream);

/* K' of every record, in place: d_rec_keys (uint64[n], as gf_dd_keys_device wrote it) mixed with d_codes (uint64[n]). */
int gf_um_mix_keys_device(const gf_index* idx, void* d_rec_keys, const void* d_codes, int64_t n, void* stream);

/* The message of the calling thread's last failed gf_um_* call. */
const char* gf_um_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* GF_UMI_H */
