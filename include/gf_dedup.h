/* gf_dedup — duplicate reads removed on the device, and the duplication rate: C ABI of libgfdedup.so.
 *
 * Deep cell-free-DNA panels hold many PCR duplicates, and the duplication rate is a figure a sample is accepted or
 * rejected on.  The reference collapses duplicates only at the very end, per fusion and by position
 * (FusionResult::calc_unique); until then every copy is merged, mapped, named and reported.  These calls find the
 * duplicates among records that already sit in HBM, behind the read filter (gf_read_filter.h) and in front of a scan,
 * with a hash table in HBM that the caller owns and that lives across calls.  A feature outside the reference, and
 * nothing calls it unless asked to.
 *
 * The predicate.  A record is its bases b[0..L), L = max(off[i + 1] - off[i], 0), at any length, also above
 * GF_MAX_READ_LEN; the qualities play no part.  Arithmetic is mod 2^64.
 *   fold(c) = c & 0xDF: the cases of a letter fold, and so do a few other byte pairs ('N' and 'n', ..).
 *   word j (j < ceil(L / 8)) is bytes 8 j .. 8 j + 7 folded, little-endian, with bytes at or past L as 0.
 *   mix(x): x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31.
 *   H(record) = mix(L + sum over j of mix(w_j + (j + 1) 0x9E3779B97F4A7C15)); H of no bases is 0.
 *   key of a single-end read: K = H(r); of a pair: K = mix(H(r1) + mix(H(r2) + 1)).  A K of 0 becomes 1.
 *   a record with no bases (for a pair: L1 + L2 == 0) is never hashed, never inserted, never a duplicate, and stays
 *   empty; its key is written as 0.
 * Known answers: K("ACGT") = K("acgt") = 0xab0fcab10dd0c6f9, K("ACGT", "") = 0xade372bd9e169438.
 * The sum over the words does not depend on their order, so the lanes of a group each take words and add.
 *
 * Two records are duplicates when their keys are equal.  Of the records with one key the one with the lowest global
 * index stays: the position in file order over everything the table has been offered (first_index + i).  Every other
 * record with that key is a duplicate and becomes a record of length 0, with its mate.  Record count, order and
 * indices stay, so names and original records are those of the sequencer, as with the filter.
 *
 * A 64-bit key wrongly joins two distinct records with probability about n^2 / 2^65: 3e-4 expected false joins for
 * 1e8 pairs.  This is fastp's trade, with a wider key.
 *
 * The table is three caller-owned device arrays of `slots` entries, slots a power of two and at least
 * GF_DD_MIN_SLOTS: keys (uint64, 0 = empty), first (int64, the lowest global index seen for the key, INT64_MAX =
 * empty) and count (uint32, how often the key was offered; may be NULL, and then nothing is counted).  A key's home
 * slot is K & (slots - 1) and the probe goes to the next slot, wrapping.  The layout inside the arrays is not
 * contract; the set of (key, first, count) is.  An empty table is keys and count zeroed and first filled with
 * INT64_MAX.  A table should stay at most half full: the caller grows it with gf_dd_rehash_device.
 *
 * A library of its own on top of libgfmatch.so (it uses gf_index_info_get of gfmatch.h to find the index's device).
 * Conventions are those of gfmatch.h: plain pointers and sizes, caller owns every buffer, GF_OK or a negative GF_ERR_*
 * code, with a message for the calling thread in gf_dd_last_error().  Every device call is one asynchronous call
 * queued on `stream` (a hipStream_t, NULL = default stream): no host synchronisation, no allocation by this library
 * and no copy between host and device.  There is no CPU fallback: host memory is refused (GF_ERR_NO_DEVICE).  As in
 * gfmatch.h the kernels load whole aligned 16-byte chunks around a record: up to 15 bytes before its first and past
 * its last byte are READ (never written, never interpreted).  Deterministic: every sum and every min is an integer.
 */
#ifndef GF_DEDUP_H
#define GF_DEDUP_H

#include "gfmatch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GF_DD_LEVELS 32
#define GF_DD_TOTALS 6
#define GF_DD_MIN_SLOTS 1024

/* d_totals (int64[GF_DD_TOTALS]) is ADDED into, never zeroed: [0] records offered, [1] records hashed (non-empty),
 * [2] keys new in this call, [5] failed probes — by gf_dd_insert_device; [3] duplicates, [4] bases removed (both
 * mates') — by gf_dd_remove_device.  [3] is [1] - [2] when first_index only ever grows. */

/* K of every record: d_rec_keys (uint64[n]), 0 for a record with no bases.  d_l_bases (uint8) and d_l_off
 * (int64[n + 1], as gf_fastq_gather_device writes it; need not start at 0): record i is bytes d_l_off[i] ..
 * d_l_off[i + 1].  d_r_bases / d_r_off: the mates, both NULL for single-end input. */
int gf_dd_keys_device(const gf_index* idx, const void* d_l_bases, const void* d_l_off, const void* d_r_bases,
                      const void* d_r_off, int64_t n, void* d_rec_keys, void* stream);

/* Every non-zero key of d_rec_keys (uint64[n]) found or placed in the table; first[s] = min(first[s],
 * first_index + i); with d_count, count[s] += 1; d_rec_slot (int64[n]): the slot s of record i, -1 for key 0 and for
 * a probe that visited `slots` entries without success (counted in d_totals[5]; it never spins). */
int gf_dd_insert_device(const gf_index* idx, const void* d_rec_keys, int64_t n, int64_t first_index, void* d_keys,
                        void* d_first, void* d_count, int64_t slots, void* d_rec_slot, void* d_totals, void* stream);

/* Device bytes gf_dd_remove_device needs as d_workspace for n records.  Non-decreasing in n. */
int64_t gf_dd_workspace_bytes(int64_t n);

/* The duplicates emptied: record i is a duplicate when d_rec_slot[i] >= 0 and first[d_rec_slot[i]] !=
 * first_index + i.  To be queued behind the insert of the same records.  Input as gf_pp_filter_device takes it (bases,
 * qualities at the bases' offsets, offsets; the mates' three NULL for single-end input); output as it writes it: the
 * survivors back to back in d_*_out_bases / d_*_out_quals (as many bytes as the records had), record i at
 * d_*_out_off[i] .. d_*_out_off[i + 1] (int64[n + 1], from 0).  d_dup (uint8[n]): 1 for a duplicate.
 * d_workspace: gf_dd_workspace_bytes(n) bytes (GF_ERR_CAPACITY when smaller). */
int gf_dd_remove_device(const gf_index* idx, const void* d_l_bases, const void* d_l_quals, const void* d_l_off,
                        const void* d_r_bases, const void* d_r_quals, const void* d_r_off, int64_t n,
                        int64_t first_index, const void* d_rec_slot, const void* d_first, void* d_workspace,
                        int64_t workspace_bytes, void* d_l_out_bases, void* d_l_out_quals, void* d_l_out_off,
                        void* d_r_out_bases, void* d_r_out_quals, void* d_r_out_off, void* d_dup, void* d_totals,
                        void* stream);

/* Every occupied entry of the old table placed in the new one, which this call empties first.  Only growing:
 * new_slots > old_slots (GF_ERR_ARG otherwise).  A NULL count on either side: nothing is carried over. */
int gf_dd_rehash_device(const gf_index* idx, const void* d_old_keys, const void* d_old_first, const void* d_old_count,
                        int64_t old_slots, void* d_new_keys, void* d_new_first, void* d_new_count, int64_t new_slots,
                        void* stream);

/* ADDS into d_hist (int64[GF_DD_LEVELS]): entry c the keys offered c times, 1 <= c <= 30; entry 31 the keys offered
 * 31 times or more; entry 0 stays as it is. */
int gf_dd_histogram_device(const gf_index* idx, const void* d_keys, const void* d_count, int64_t slots, void* d_hist,
                           void* stream);

/* The message of the calling thread's last failed gf_dd_* call. */
const char* gf_dd_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* GF_DEDUP_H */
