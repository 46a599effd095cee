/* gf_alignable — the whole-genome alignable filter: C ABI of libgfalign.so.
 *
 * The last false-positive filter of the pipeline, as a filter that works: a candidate read that lies
 * end to end somewhere in the reference is no evidence of a fusion.  The predicate: for a strand of the read (the read
 * as it is, or its reverse complement: anything outside ACGTacgt becomes N, upper case), a contig and a start p with
 * the whole strand inside the contig, position i matches when the strand's byte equals the contig's, upper-cased, and
 * is one of ACGT; it is covered when it lies in a window of GF_AL_WINDOW positions that all match.  The read is
 * alignable when on some such diagonal fewer than GF_AL_UNCOVERED_LIMIT positions are uncovered.  The diagonal is
 * exact: no indels.
 *
 * Three steps, each one asynchronous call:
 *   gf_al_seeds_device   the reads -> their two strands, a seed {key, strand string, offset} per valid 16-mer in the slot
 *                        of its first base, and a membership filter over the keys (no false negatives)
 *   (the caller sorts the slots ascending as int64: a slot without a seed is INT64_MAX and sorts last)
 *   gf_al_index_device   the sorted slots -> where each bucket of keys starts
 *   gf_al_scan_device    one piece of reference text -> the bit of every read that is alignable inside it, ORed into
 *                        the flags; called once per piece, the flags zeroed by the caller before the first
 *
 * A piece is dense text: contigs back to back with one GF_AL_SEPARATOR byte between two of them (no alignment holds a
 * separator), upper-cased on the fly.  A contig cut into several pieces must overlap by the longest read's length less
 * one, so that every alignment lies whole in one piece.
 *
 * No gf_index is taken: the device is that of the pointers.  The library is built next to libgfmatch.so and links
 * against it like its siblings, but calls nothing of it on the device.  Conventions are those of gfmatch.h: plain
 * pointers and sizes, caller owns every buffer, GF_OK or a negative GF_ERR_* code, with a message for the calling thread
 * in gf_al_last_error().  The device calls are queued on `stream` (a hipStream_t, NULL = default stream): no host
 * synchronisation, no allocation, no copy between host and device.
 */
#ifndef GF_ALIGNABLE_H
#define GF_ALIGNABLE_H

#include "gfmatch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GF_AL_WINDOW 16            /* matcher.rs:30 */
#define GF_AL_UNCOVERED_LIMIT 10   /* matcher.rs:516 */
#define GF_AL_READS_MAX 262144     /* reads per call: a seed names its strand string in 19 bits */
#define GF_AL_FILTER_LOG2_MIN 16   /* the filter has 2^16 .. 2^32 bits; 2^32 is the exact map of all keys */
#define GF_AL_FILTER_LOG2_MAX 32
#define GF_AL_SEPARATOR_BYTE 0

/* Sizes of the caller's buffers, in bytes; 0 for an argument out of range. */
int64_t gf_al_filter_bytes(int32_t filter_log2_bits); /* d_filter */
int64_t gf_al_bucket_bytes(void);                     /* d_bucket_start */
int64_t gf_al_flag_bytes(int64_t n_reads);            /* d_flags: uint32[ceil(n_reads / 32)], read r is bit r % 32 of
                                                         word r / 32 */

/* The seeds of n_reads reads.
 *   d_bases: uint8[bases_bytes], the reads back to back.  d_offsets: int64[n_reads + 1].  A read whose offsets point
 *   outside d_bases, or longer than GF_MAX_READ_LEN, or shorter than GF_AL_WINDOW, gets no seed: it is never flagged.
 *   d_strands: uint8[2 * bases_bytes], written: both strands of read r at 2 * d_offsets[r].
 *   d_seeds: int64[2 * bases_bytes], written: a seed or INT64_MAX per slot.
 *   d_filter: gf_al_filter_bytes(filter_log2_bits), zeroed and written. */
int gf_al_seeds_device(const void* d_bases, int64_t bases_bytes, const void* d_offsets, int64_t n_reads, void* d_strands,
                       void* d_seeds, void* d_filter, int32_t filter_log2_bits, void* stream);

/* d_seeds: the int64[n_slots] of gf_al_seeds_device, sorted ascending.  d_bucket_start: gf_al_bucket_bytes(), written. */
int gf_al_index_device(const void* d_seeds, int64_t n_slots, void* d_bucket_start, void* stream);

/* One piece of reference text against the seeds.
 *   d_text: uint8[text_bytes], aligned to 16 bytes.
 *   d_strands, bases_bytes, d_offsets, n_reads, d_filter, filter_log2_bits: those of gf_al_seeds_device; d_seeds (sorted)
 *   and d_bucket_start: those of gf_al_index_device.
 *   d_flags: gf_al_flag_bytes(n_reads); bits are only ever set.  A read whose bit is set is not tested again. */
int gf_al_scan_device(const void* d_text, int64_t text_bytes, const void* d_strands, int64_t bases_bytes,
                      const void* d_offsets, int64_t n_reads, const void* d_seeds, const void* d_bucket_start,
                      const void* d_filter, int32_t filter_log2_bits, void* d_flags, void* stream);

/* The message of the calling thread's last failed gf_al_* call. */
const char* gf_al_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* GF_ALIGNABLE_H */
